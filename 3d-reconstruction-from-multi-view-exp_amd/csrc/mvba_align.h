// Similarity alignment of two point sets (mvba_align_robust, mvba_align, mvba_align_sample): y ~ s Q x + tau by 3-point RANSAC and
// by plain least squares -- kernels and host code, gfx950.
//
// Included by mvba.hip after mvba_tri_ransac.h: uses mvba_ransac_host.h's align_solve, argument checks, RsTile (the call is a tile
// of one item), rs_stop, rs_current, rs_other, RsLaps and state bits, mvba_ransac.h's rs_sample, sample_entry, rs_score_block,
// rs_score_add, k_ransac_scan and RS_HYP_BLOCK, mvba_twoview.h's tv_combine, mvba_init.h's init_finite, mvba_start.h's chunk_sum,
// chunk_ballot, chunk_total, chunk_rank, mask_step, InitClock and START_CHUNK, and mvba.hip's DevBufs, fail and MVBA_HIP.  Nothing
// here runs on the LM path.  
//
// The usable correspondences (ok allows them, six finite numbers) are compacted into a dense array of (x, y), 48 bytes each, in
// ascending order -- chunk counts, k_ransac_scan, ballot and prefix -- with their row numbers beside them; every later pass reads
// that array.  One THREAD per hypothesis draws 3 indices and solves Horn's 4 x 4 eigen-problem in registers (align_solve: no LDS,
// no scratch).  The scoring kernel holds one correspondence per thread in registers and walks ALL hypothesis blocks of 64, each
// staged in LDS (64 x 12 doubles = 6 KiB): a correspondence is read once.  A hypothesis's inliers of a wave are one ballot and
// one popcount, then integer atomics (LDS, then device memory): exact in any order.  A refit sums the moments of the compacted
// array under a byte mask in two passes (the centroids, then the centred second moments: chunk_sum, then k_twoview_combine) and
// align_solve runs on the host.  No floating-point atomics.

namespace {

constexpr int AL_MIN = 3;  // correspondences of a sample, and the fewest a fit takes

struct AlCentre {
  double x[3], y[3];
};

// row a of (src, dst) -> z = (x, y); false if it is past the end, ok forbids it or a number is not finite
__device__ __forceinline__ bool al_usable(long long a, long long n, const double *__restrict__ src, const double *__restrict__ dst,
                                          const unsigned char *__restrict__ ok, double (&z)[6]) {
  if (a >= n || (ok && !ok[a])) return false;
  bool fin = true;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    z[e] = src[3 * a + e];
    z[3 + e] = dst[3 * a + e];
    fin = fin && init_finite(z[e]) && init_finite(z[3 + e]);
  }
  return fin;
}

__device__ __forceinline__ void al_load(const double2 *__restrict__ comp, long long j, double (&z)[6]) {
  const double2 a = comp[3 * j], b = comp[3 * j + 1], c = comp[3 * j + 2];
  z[0] = a.x; z[1] = a.y; z[2] = b.x; z[3] = b.y; z[4] = c.x; z[5] = c.y;
}

// |sQ x + tau - y|^2 under the model m = (sQ row-major, tau)
__device__ __forceinline__ double al_dist2(const double *m, const double (&z)[6]) {
  double d2 = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double d = m[3 * a] * z[0] + m[3 * a + 1] * z[1] + m[3 * a + 2] * z[2] + m[9 + a] - z[3 + a];
    d2 += d * d;
  }
  return d2;
}

// |(p1 - p0) x (p2 - p0)|^2 / (|p1 - p0|^2 |p2 - p0|^2) of a triple: the sine squared of its angle at p0 (NaN if two coincide)
RS_HD_INLINE double al_pivot(const double (&p)[3][3]) {
  const double a[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]}, b[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
  const double c0 = a[1] * b[2] - a[2] * b[1], c1 = a[2] * b[0] - a[0] * b[2], c2 = a[0] * b[1] - a[1] * b[0];
  return (c0 * c0 + c1 * c1 + c2 * c2) / ((a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) * (b[0] * b[0] + b[1] * b[1] + b[2] * b[2]));
}

// The similarity through three correspondences: centre both triples, sum their moments, align_solve.  false (sim13 NaN) if
// either triple is collinear or coincident to the relative pivot, or align_solve refuses.
RS_HD_INLINE bool al_hypothesis(const double (&x)[3][3], const double (&y)[3][3], bool with_scale, double (&sim13)[13]) {
  double mx[3], my[3], mom[11], gap;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    mx[e] = (x[0][e] + x[1][e] + x[2][e]) / 3.0;
    my[e] = (y[0][e] + y[1][e] + y[2][e]) / 3.0;
  }
#pragma unroll
  for (int e = 0; e < 11; ++e) mom[e] = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double xc[3] = {x[c][0] - mx[0], x[c][1] - mx[1], x[c][2] - mx[2]}, yc[3] = {y[c][0] - my[0], y[c][1] - my[1], y[c][2] - my[2]};
    mom[0] += xc[0] * xc[0] + xc[1] * xc[1] + xc[2] * xc[2];
    mom[1] += yc[0] * yc[0] + yc[1] * yc[1] + yc[2] * yc[2];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) mom[2 + 3 * a + b] += yc[a] * xc[b];
  }
  const bool spread = al_pivot(x) > INIT_REL_PIVOT && al_pivot(y) > INIT_REL_PIVOT;  // (NaN fails)
  return align_solve(mx, my, mom, with_scale, sim13, gap) == 0 && spread;
}

// cnt[chunk] = the number of usable correspondences among the chunk's 256
__global__ __launch_bounds__(START_CHUNK) void k_align_count(long long n, const double *__restrict__ src, const double *__restrict__ dst,
                                                             const unsigned char *__restrict__ ok, int *__restrict__ cnt) {
  __shared__ int s_w[START_CHUNK / 64];
  const int i = threadIdx.x;
  double z[6];
  chunk_ballot(al_usable((long long)blockIdx.x * START_CHUNK + i, n, src, dst, ok, z), s_w);
  if (i == 0) cnt[blockIdx.x] = chunk_total(s_w);
}

// comp[j] = (x, y) and id[j] = the row of the j-th usable correspondence, ascending (off: the exclusive scan of the chunk counts)
__global__ __launch_bounds__(START_CHUNK) void k_align_compact(long long n, const double *__restrict__ src, const double *__restrict__ dst,
                                                               const unsigned char *__restrict__ ok, const int *__restrict__ off,
                                                               double2 *__restrict__ comp, int *__restrict__ id) {
  __shared__ int s_w[START_CHUNK / 64];
  const int i = threadIdx.x;
  const long long a = (long long)blockIdx.x * START_CHUNK + i;
  double z[6];
  const bool use = al_usable(a, n, src, dst, ok, z);
  const unsigned long long b = chunk_ballot(use, s_w);
  if (!use) return;
  const long long j = off[blockIdx.x] + chunk_rank(b, s_w);
  comp[3 * j] = make_double2(z[0], z[1]);  // (j < the usable count <= n)
  comp[3 * j + 1] = make_double2(z[2], z[3]);
  comp[3 * j + 2] = make_double2(z[4], z[5]);
  id[j] = (int)a;
}

// One thread per hypothesis, in registers: hyp[h] = (sQ, tau), hyp_s[h] = s, hyp_count[h] = 0; NaN and -1 if degenerate
__global__ __launch_bounds__(RS_HYP_BLOCK) void k_align_hyp(int H, unsigned long long seed, const int *__restrict__ ntot,
                                                            const double2 *__restrict__ comp, int with_scale, double *__restrict__ hyp,
                                                            double *__restrict__ hyp_s, int *__restrict__ hyp_count) {
  const int h = blockIdx.x * RS_HYP_BLOCK + threadIdx.x;
  if (h >= H) return;
  const int n = ntot[0];
  double sim[13];
  bool good = n >= AL_MIN;  // (below 3 the rejection loop of rs_sample would not end)
  if (good) {
    long long idx[AL_MIN];
    rs_sample(seed, 0, 0, h, n, idx);
    double x[3][3], y[3][3];
#pragma unroll
    for (int c = 0; c < AL_MIN; ++c) {
      double z[6];
      al_load(comp, idx[c], z);
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        x[c][e] = z[e];
        y[c][e] = z[3 + e];
      }
    }
    good = al_hypothesis(x, y, with_scale != 0, sim);
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) hyp[12 * (size_t)h + e] = good ? sim[0] * sim[1 + e] : NAN;
#pragma unroll
  for (int e = 0; e < 3; ++e) hyp[12 * (size_t)h + 9 + e] = good ? sim[10 + e] : NAN;
  hyp_s[h] = good ? sim[0] : NAN;
  hyp_count[h] = good ? 0 : -1;
}

// Scoring: one workgroup per chunk of compacted correspondences, one correspondence per thread; the workgroup walks the blocks
// of 64 hypotheses through LDS (every lane reads the same address: a broadcast).  A degenerate hypothesis is NaN: nothing
// passes, its count stays -1.
__global__ __launch_bounds__(START_CHUNK) void k_align_score(int H, const int *__restrict__ ntot, const double2 *__restrict__ comp,
                                                             const double *__restrict__ hyp, double thr2, int *__restrict__ hyp_count) {
  __shared__ double s_m[RS_HYP_BLOCK * 12];
  __shared__ int s_cnt[RS_HYP_BLOCK];
  const int i = threadIdx.x, lane = i & 63, n = ntot[0];
  const long long j = (long long)blockIdx.x * START_CHUNK + i;
  if (n < AL_MIN || (long long)blockIdx.x * START_CHUNK >= n) return;  // (the whole workgroup leaves)
  const bool live = j < n;
  double z[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (live) al_load(comp, j, z);
  for (int h0 = 0; h0 < H; h0 += RS_HYP_BLOCK) {
    const int nh = min(RS_HYP_BLOCK, H - h0);
    for (int e = i; e < nh * 12; e += START_CHUNK) s_m[e] = hyp[12 * (size_t)h0 + e];
    if (i < RS_HYP_BLOCK) s_cnt[i] = 0;
    __syncthreads();
    const int mine = rs_score_block(nh, lane, live, [&](int hh) { return al_dist2(s_m + 12 * hh, z) <= thr2; });
    // (its barrier also: every read of s_m is done before the next block is staged; s_cnt[i] is read and reset by thread i)
    rs_score_add(mine, nh, lane, s_cnt, hyp_count + h0);
  }
}

// The inlier bytes of the model m = (sQ, tau) over the compacted array into inl, and part[chunk][2] = (count, sum of d^2 over
// it) by the tree of chunk_sum (the count is exact in a double)
__global__ __launch_bounds__(START_CHUNK) void k_align_mask(const int *__restrict__ ntot, const double2 *__restrict__ comp,
                                                            const double *__restrict__ m, double thr2, unsigned char *__restrict__ inl,
                                                            double *__restrict__ part) {
  __shared__ double s_w[START_CHUNK / 64][2];
  const long long j = (long long)blockIdx.x * START_CHUNK + threadIdx.x;
  double v[2] = {0.0, 0.0};
  if (j < ntot[0]) {
    double z[6];
    al_load(comp, j, z);
    const double d2 = al_dist2(m, z);
    mask_step(d2 <= thr2, d2, &inl[j], v);
  }
  chunk_sum<2>(v, s_w, part + (size_t)blockIdx.x * 2);
}

// The two passes of a fit over the compacted correspondences whose byte in inl is set (inl == nullptr: all of them):
// PASS 0: part[chunk][7] = (count, sum x, sum y); PASS 1: part[chunk][11] = (sum |x_c|^2, sum |y_c|^2, sum y_c x_c^T) about c.
template <int PASS>
__global__ __launch_bounds__(START_CHUNK) void k_align_moments(const int *__restrict__ ntot, const double2 *__restrict__ comp,
                                                               const unsigned char *__restrict__ inl, AlCentre c, double *__restrict__ part) {
  constexpr int NV = PASS == 0 ? 7 : 11;
  __shared__ double s_w[START_CHUNK / 64][NV];
  const long long j = (long long)blockIdx.x * START_CHUNK + threadIdx.x;
  double v[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) v[e] = 0.0;
  if (j < ntot[0] && (!inl || inl[j])) {
    double z[6];
    al_load(comp, j, z);
    if constexpr (PASS == 0) {
      v[0] = 1.0;
#pragma unroll
      for (int e = 0; e < 6; ++e) v[1 + e] = z[e];
    } else {
      const double xc[3] = {z[0] - c.x[0], z[1] - c.x[1], z[2] - c.x[2]}, yc[3] = {z[3] - c.y[0], z[4] - c.y[1], z[5] - c.y[2]};
      v[0] = xc[0] * xc[0] + xc[1] * xc[1] + xc[2] * xc[2];
      v[1] = yc[0] * yc[0] + yc[1] * yc[1] + yc[2] * yc[2];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) v[2 + 3 * a + b] = yc[a] * xc[b];
    }
  }
  chunk_sum<NV>(v, s_w, part + (size_t)blockIdx.x * NV);
}

// out[row] = 1 for the compacted correspondences whose byte in inl is set (out is zero beforehand)
__global__ __launch_bounds__(START_CHUNK) void k_align_scatter(const int *__restrict__ ntot, const int *__restrict__ id,
                                                               const unsigned char *__restrict__ inl, unsigned char *__restrict__ out) {
  const long long j = (long long)blockIdx.x * START_CHUNK + threadIdx.x;
  if (j < ntot[0] && inl[j]) out[id[j]] = 1;
}

// The device side of one alignment call: the compacted correspondences and what the passes over them need.
struct AlignDev {
  DevBufs tmp;  // (freed on every return)
  int n_usable = 0;
  long long n_in = 0;  // chunks of the input rows
  unsigned n_ch = 1;   // chunks of the compacted array
  double *dsrc = nullptr, *ddst = nullptr;
  unsigned char *dok = nullptr;
  int *doff = nullptr, *dntot = nullptr, *did = nullptr;
  double2 *dcomp = nullptr;
  double *dpart = nullptr, *dS = nullptr, *dmodel = nullptr;
  unsigned char *dinl[2] = {nullptr, nullptr};

  // the inputs to the device, and the buffers whose size they fix
  int upload(int64_t n, const double *src, const double *dst, const uint8_t *ok) {
    n_in = (n + START_CHUNK - 1) / START_CHUNK;
    int rc;
    if ((rc = tmp.alloc(&dsrc, 3 * (size_t)n)) || (rc = tmp.alloc(&ddst, 3 * (size_t)n)) || (rc = tmp.alloc(&doff, (size_t)n_in)) ||
        (rc = tmp.alloc(&dntot, 1)) || (rc = tmp.alloc(&did, (size_t)n)) || (rc = tmp.alloc(&dcomp, 3 * (size_t)n)) ||
        (rc = tmp.alloc(&dS, 11)) || (rc = tmp.alloc(&dmodel, 12)))
      return rc;
    if (ok && (rc = tmp.alloc(&dok, (size_t)n))) return rc;
    MVBA_HIP(hipMemcpy(dsrc, src, sizeof(double) * 3 * n, hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(ddst, dst, sizeof(double) * 3 * n, hipMemcpyHostToDevice));
    if (ok) MVBA_HIP(hipMemcpy(dok, ok, (size_t)n, hipMemcpyHostToDevice));
    return MVBA_OK;
  }

  // compaction, then the buffers of the passes over the compacted array (masks: the two byte masks a robust call alternates between)
  int compact(int64_t n, bool masks) {
    const dim3 gin((unsigned)n_in), bch(START_CHUNK);
    hipLaunchKernelGGL(k_align_count, gin, bch, 0, 0, (long long)n, dsrc, ddst, dok, doff);
    hipLaunchKernelGGL(k_ransac_scan, dim3(1), dim3(256), 0, 0, (int)n_in, doff, dntot);
    hipLaunchKernelGGL(k_align_compact, gin, bch, 0, 0, (long long)n, dsrc, ddst, dok, doff, dcomp, did);
    MVBA_HIP(hipGetLastError());
    MVBA_HIP(hipMemcpy(&n_usable, dntot, sizeof(int), hipMemcpyDeviceToHost));
    tmp.release(dsrc);
    tmp.release(ddst);
    n_ch = (unsigned)std::max<long long>(1, ((long long)n_usable + START_CHUNK - 1) / START_CHUNK);
    int rc;
    if ((rc = tmp.alloc(&dpart, 11 * (size_t)n_ch))) return rc;
    if (masks && ((rc = tmp.alloc(&dinl[0], (size_t)n_usable)) || (rc = tmp.alloc(&dinl[1], (size_t)n_usable)))) return rc;
    return MVBA_OK;
  }

  // nv sums of the chunk partials -> out, in k_twoview_combine's order
  int sums(int nv, double *out) {
    tv_combine(1, nv, n_ch, dpart, dS, nv);
    MVBA_HIP(hipGetLastError());
    MVBA_HIP(hipMemcpy(out, dS, sizeof(double) * nv, hipMemcpyDeviceToHost));
    return MVBA_OK;
  }

  // the centred moments of the correspondences under inl (nullptr: all): the count, the centroids and align_solve's mom
  int moments(const unsigned char *inl, double &count, AlCentre &c, double (&mom)[11]) {
    double s7[7];
    int rc;
    hipLaunchKernelGGL(k_align_moments<0>, dim3(n_ch), dim3(START_CHUNK), 0, 0, dntot, dcomp, inl, AlCentre{}, dpart);
    if ((rc = sums(7, s7))) return rc;
    count = s7[0];
    for (int e = 0; e < 3; ++e) {
      c.x[e] = s7[1 + e] / count;
      c.y[e] = s7[4 + e] / count;
    }
    hipLaunchKernelGGL(k_align_moments<1>, dim3(n_ch), dim3(START_CHUNK), 0, 0, dntot, dcomp, inl, c, dpart);
    return sums(11, mom);
  }

  // the least-squares similarity of the correspondences under inl: *st = align_solve's status
  int fit(const unsigned char *inl, bool with_scale, double (&sim13)[13], double &gap, int *st) {
    double count, mom[11];
    AlCentre c;
    int rc;
    if ((rc = moments(inl, count, c, mom))) return rc;
    *st = align_solve(c.x, c.y, mom, with_scale, sim13, gap);
    return MVBA_OK;
  }

  // the inliers of the model `m` on the device (sQ, tau) into inl: s2 = (their number, their sum of d^2)
  int mask(const double *m, double thr2, unsigned char *inl, double (&s2)[2]) {
    hipLaunchKernelGGL(k_align_mask, dim3(n_ch), dim3(START_CHUNK), 0, 0, dntot, dcomp, m, thr2, inl, dpart);
    return sums(2, s2);
  }

  // sim13 -> the 12 doubles the mask kernel reads, at dmodel
  int set_model(const double (&sim13)[13]) {
    double m[12];
    for (int e = 0; e < 9; ++e) m[e] = sim13[0] * sim13[1 + e];
    for (int e = 0; e < 3; ++e) m[9 + e] = sim13[10 + e];
    MVBA_HIP(hipMemcpy(dmodel, m, sizeof(m), hipMemcpyHostToDevice));
    return MVBA_OK;
  }
};

int align_check(int64_t n, const double *src, const double *dst, const double *sim13, int sim_arg) {
  if (!src || !dst || !sim13)
    return fail(MVBA_ERR_BADARG, std::string("null argument: ") + (!src ? "src" : (!dst ? "dst" : "sim13")) + " (argument " +
                                     std::to_string(!src ? 2 : (!dst ? 3 : sim_arg)) + ")");
  if (n < 0 || n >= (1LL << 31)) return fail(MVBA_ERR_BADARG, "n = " + std::to_string(n) + " must be in 0 .. 2^31 - 1");
  return MVBA_OK;
}

}  // namespace

extern "C" {

int mvba_align_sample(uint64_t seed, int32_t h, int64_t n, int64_t *idx3) {
  return sample_entry<AL_MIN>(seed, "h", 0, 0, h, n, idx3, "idx3", 4);
}

int mvba_align_robust(int64_t n, const double *src, const double *dst, const uint8_t *ok, int32_t with_scale, double threshold,
                      int32_t n_hypotheses, uint64_t seed, int32_t n_refit, double *sim13, double *quality, int64_t *n_usable,
                      int64_t *n_inliers, int32_t *best, uint8_t *inlier, int32_t *hyp_count, int32_t *status, double *timings_ms,
                      int32_t device) {
  int rc;
  if ((rc = align_check(n, src, dst, sim13, 10)) || (rc = rs_check_search(threshold, n_hypotheses)) || (rc = rs_check_refit(n_refit))) return rc;
  const int H = n_hypotheses;
  const double thr2 = threshold * threshold;
  // the defaults are those of a call without usable correspondences: status 1
  for (int e = 0; e < 13; ++e) sim13[e] = NAN;
  if (quality) quality[0] = quality[1] = quality[2] = NAN;  // (three figures, not RsTile's two: written here)
  RsTile::defaults(1, H, status, best, hyp_count, n_usable, n_inliers, nullptr);
  if (inlier) std::memset(inlier, 0, (size_t)n);
  if (timings_ms) timings_ms[0] = timings_ms[1] = timings_ms[2] = timings_ms[3] = 0.0;
  if (n == 0) return MVBA_OK;

  if (device >= 0) MVBA_HIP(hipSetDevice(device));
  InitClock clk;
  RsLaps laps;
  AlignDev d;
  double *dhyp = nullptr, *dhs = nullptr;
  int *dhc = nullptr;
  unsigned char *dout = nullptr;
  if ((rc = d.upload(n, src, dst, ok)) || (rc = d.tmp.alloc(&dhyp, 12 * (size_t)H)) || (rc = d.tmp.alloc(&dhs, (size_t)H)) ||
      (rc = d.tmp.alloc(&dhc, (size_t)H)))
    return rc;
  laps.upload = clk.lap();
  if ((rc = d.compact(n, true))) return rc;
  if (n_usable) *n_usable = d.n_usable;

  hipLaunchKernelGGL(k_align_hyp, dim3((H + RS_HYP_BLOCK - 1) / RS_HYP_BLOCK), dim3(RS_HYP_BLOCK), 0, 0, H, (unsigned long long)seed, d.dntot, d.dcomp,
                     (int)with_scale, dhyp, dhs, dhc);
  hipLaunchKernelGGL(k_align_score, dim3(d.n_ch), dim3(START_CHUNK), 0, 0, H, d.dntot, d.dcomp, dhyp, thr2, dhc);
  MVBA_HIP(hipGetLastError());
  std::vector<int> hc((size_t)H);
  MVBA_HIP(hipMemcpy(hc.data(), dhc, sizeof(int) * H, hipMemcpyDeviceToHost));
  laps.score = clk.lap();

  // the call is a tile of one item
  RsTile t(1);
  int state = 0;
  double sim[13], gap = 0.0, s2[2];
  auto write = [&]() {
    t.write(0, status, best, hyp_count, n_inliers, nullptr, [&](int) {
      std::copy(sim, sim + 13, sim13);
      return gap;
    });
  };
  t.pick(1, &state, hc.data(), H, &d.n_usable, AL_MIN);
  if (t.st[0]) {
    write();
    laps.other = clk.lap();
    laps.write(timings_ms);
    return MVBA_OK;
  }
  // the best hypothesis as the device holds it
  double m12[12];
  const double *dbest = dhyp + 12 * (size_t)t.best[0];
  MVBA_HIP(hipMemcpy(m12, dbest, sizeof(m12), hipMemcpyDeviceToHost));
  MVBA_HIP(hipMemcpy(&sim[0], dhs + t.best[0], sizeof(double), hipMemcpyDeviceToHost));
  for (int e = 0; e < 9; ++e) sim[1 + e] = m12[e] / sim[0];
  for (int e = 0; e < 3; ++e) sim[10 + e] = m12[9 + e];
  if ((rc = d.mask(dbest, thr2, rs_other(state, d.dinl[0], d.dinl[1]), s2))) return rc;
  t.first(s2, [](int) { return 0; });
  laps.other = clk.lap();

  // refits: the least-squares fit of the current inliers alone; the first is kept if it has three inliers of its own, a later
  // one while its set does not shrink
  for (int r = 0; r < n_refit && t.n_active > 0; ++r) {
    double simr[13], gr;
    int st;
    if ((rc = d.fit(rs_current(state, d.dinl[0], d.dinl[1]), with_scale != 0, simr, gr, &st))) return rc;
    if (st) {
      rs_stop(state, t.n_active);
      break;
    }
    if ((rc = d.set_model(simr)) || (rc = d.mask(d.dmodel, thr2, rs_other(state, d.dinl[0], d.dinl[1]), s2))) return rc;
    t.accept(r, s2, AL_MIN, [&](int) {
      gap = gr;
      std::copy(simr, simr + 13, sim);
    });
  }
  laps.refit = clk.lap();

  const unsigned char *fin = rs_current(state, d.dinl[0], d.dinl[1]);
  double count, mom[11];
  AlCentre ctr;
  if ((rc = d.moments(fin, count, ctr, mom))) return rc;  // the spread of the final inliers
  if (inlier) {
    if ((rc = d.tmp.alloc(&dout, (size_t)n))) return rc;
    MVBA_HIP(hipMemset(dout, 0, (size_t)n));
    hipLaunchKernelGGL(k_align_scatter, dim3(d.n_ch), dim3(START_CHUNK), 0, 0, d.dntot, d.did, fin, dout);
    MVBA_HIP(hipGetLastError());
    MVBA_HIP(hipMemcpy(inlier, dout, (size_t)n, hipMemcpyDeviceToHost));
  }
  write();
  if (quality) {
    quality[0] = sqrt(t.ssq[0] / (double)t.nin[0]);
    quality[1] = gap;
    quality[2] = mom[0] / count;
  }
  laps.other += clk.lap();
  laps.write(timings_ms);
  return MVBA_OK;
}

int mvba_align(int64_t n, const double *src, const double *dst, const uint8_t *ok, int32_t with_scale, double *sim13, double *quality,
               int64_t *n_usable, int32_t *status, int32_t device) {
  int rc;
  if ((rc = align_check(n, src, dst, sim13, 6))) return rc;
  for (int e = 0; e < 13; ++e) sim13[e] = NAN;
  if (quality) quality[0] = quality[1] = quality[2] = NAN;
  if (n_usable) *n_usable = 0;
  if (status) *status = 1;
  if (n == 0) return MVBA_OK;
  if (device >= 0) MVBA_HIP(hipSetDevice(device));
  AlignDev d;
  if ((rc = d.upload(n, src, dst, ok)) || (rc = d.compact(n, false))) return rc;
  if (n_usable) *n_usable = d.n_usable;
  if (d.n_usable < AL_MIN) return MVBA_OK;
  double count, mom[11], sim[13], gap, s2[2];
  AlCentre c;
  if ((rc = d.moments(nullptr, count, c, mom))) return rc;
  const int st = align_solve(c.x, c.y, mom, with_scale != 0, sim, gap);
  if (status) *status = st;
  if (st) return MVBA_OK;
  // the residual of every usable correspondence: the mask pass with no threshold
  unsigned char *dall = nullptr;
  if ((rc = d.tmp.alloc(&dall, (size_t)d.n_usable)) || (rc = d.set_model(sim)) || (rc = d.mask(d.dmodel, HUGE_VAL, dall, s2))) return rc;
  std::copy(sim, sim + 13, sim13);
  if (quality) {
    quality[0] = sqrt(s2[1] / count);
    quality[1] = gap;
    quality[2] = mom[0] / count;
  }
  return MVBA_OK;
}

}  // extern "C"
