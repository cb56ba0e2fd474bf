// Robust two-view geometry (mvba_two_view_robust, mvba_ransac_sample): 8-point RANSAC for the fundamental matrix -- kernels
// and host code, gfx950.
//
// Included by mvba.hip after mvba_twoview.h: uses mvba_ransac_host.h's argument checks, RsTile, rs_stop, rs_current, rs_other,
// RsLaps, limits and state bits, mvba_twoview.h's rs_shared, tv_pass, tv_row, rs_sampson, tv_denormalise, k_twoview_combine,
// k_twoview_norm, twoview_solve_pair, tv_pair_tile, tv_combine and constants, mvba_start.h's chunk_sum, chunk_ballot,
// chunk_total, chunk_rank, mask_step, checks, upload_list, InitClock and INIT_REL_PIVOT, and mvba.hip's DevBufs, fail and
// MVBA_HIP.  Nothing here runs on the LM path.  
//
// What the later robust fits take from here (mvba_homography.h, mvba_resect_ransac.h, mvba_pose_ransac.h, mvba_align.h):
// rs_lds_eig, rs_sample and sample_entry, and the scoring loop of a block of hypotheses, rs_score_block and rs_score_add.
//
// Per pair of a tile (blockIdx.y or .z: the pair inside the tile): the shared observations are compacted into a dense array
// of (x_k, y_k, x_l, y_l) in ascending point order (per-chunk counts, an exclusive scan over the pair's chunks, ballot and
// prefix inside the workgroup); every later pass reads that array.  One THREAD per hypothesis draws its 8 indices, sums its
// 9 x 9 moment matrix in registers (static indices) and diagonalises it by cyclic Jacobi with A and V in LDS, element-major
// (element e of thread t at [e x 64 + t]: run-time row and column indices address LDS, not scratch, and a wave's 64 accesses
// fall into 64 consecutive doubles).  The scoring kernel holds 64 hypothesis matrices in LDS, one compacted point per thread;
// a hypothesis's count is ballot + popcount per wave, then integer atomics (LDS, then device memory): exact in any order.
// Refits sum the moments of the compacted array under a byte mask by tv_pass and chunk_sum, as k_twoview_chunk does; the order-9
// eigen-problem, the rank-2 step and the denormalisation are twoview_solve_pair's, on the host.  No floating-point atomics.
//
// The host loop over tiles of pairs is robust_pairs<Fit>, and the scoring and mask kernels are templates over the model a Fit
// names: the fundamental matrix here (FundFit, FundModel), the homography in mvba_homography.h.

namespace {

constexpr int RS_HYP_BLOCK = 64;      // hypotheses per workgroup of k_ransac_hyp, and per LDS block of k_ransac_score
// device bytes one pair of a tile takes per point of the scene (32 compacted observation, 4 point id, 2 masks, 1 mask by
// point, 1.42 chunk counts and partials) and per hypothesis (72 F^, 72 F, 4 count), rounded up: the tile's bound
constexpr size_t RS_POINT_BYTES = 48, RS_HYP_BYTES = 160;

// The scoring loop of a thread over a block of nh <= RS_HYP_BLOCK hypotheses: in(hh) says whether the thread's item is an
// inlier of hypothesis hh of the block (live: the thread has an item); a hypothesis's inliers of a wave are one ballot and one
// popcount, kept by the lane of the hypothesis's number.  Returns that lane's count.  Every thread of the wave calls it.
template <class In>
__device__ __forceinline__ int rs_score_block(int nh, int lane, bool live, In in) {
  int mine = 0;
  for (int hh = 0; hh < nh; ++hh) {
    const int c = __popcll(__ballot(live && in(hh)));
    if (lane == hh) mine = c;
  }
  return mine;
}

// The waves' counts of rs_score_block into hyp_count[0 .. nh), the block's counts in device memory: an LDS atomic per wave and
// hypothesis into s_cnt (zero beforehand), a barrier, one device atomic per hypothesis.  Integer sums: exact in any order.
__device__ __forceinline__ void rs_score_add(int mine, int nh, int lane, int (&s_cnt)[RS_HYP_BLOCK], int *__restrict__ hyp_count) {
  const int i = threadIdx.x;
  if (mine) atomicAdd(&s_cnt[lane], mine);
  __syncthreads();
  if (i < nh && s_cnt[i]) atomicAdd(&hyp_count[i], s_cnt[i]);
}

// The eigenvector of the smallest eigenvalue of a thread's symmetric N x N matrix by cyclic Jacobi with A and V in LDS,
// element-major: sA and sV are the thread's columns, element e at [e * RS_HYP_BLOCK].  A is filled by the caller, V is set
// to the identity here.  false if not good (v is untouched then), or if the second-smallest eigenvalue fails the pivot rule.
template <int N>
__device__ __forceinline__ bool rs_lds_eig(double *sA, double *sV, bool good, double (&v)[N]) {
  auto A = [&](int r, int c) -> double & { return sA[(r * N + c) * RS_HYP_BLOCK]; };
  auto V = [&](int r, int c) -> double & { return sV[(r * N + c) * RS_HYP_BLOCK]; };
  for (int e = 0; e < N * N; ++e) sV[e * RS_HYP_BLOCK] = (e % (N + 1) == 0) ? 1.0 : 0.0;
  // sym_eig_jacobi's rotations and stopping rule, with run-time indices into LDS
  for (int sweep = 0; sweep < 30 && good; ++sweep) {
    bool any = false;
    for (int a = 0; a < N - 1; ++a)
      for (int b = a + 1; b < N; ++b) {
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
        for (int r = 0; r < N; ++r) {
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
  if (!good) return false;
  int best = 0;
  double l1 = A(0, 0), lmax = A(0, 0), l2 = HUGE_VAL;
  for (int e = 1; e < N; ++e) {
    const double d = A(e, e);
    if (d < l1) { l1 = d; best = e; }
    lmax = fmax(lmax, d);
  }
  for (int e = 0; e < N; ++e)
    if (e != best) l2 = fmin(l2, A(e, e));
#pragma unroll
  for (int e = 0; e < N; ++e) v[e] = V(e, best);
  return l2 > INIT_REL_PIVOT * lmax;
}

__host__ __device__ __forceinline__ unsigned long long rs_mix(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the NS distinct indices below n (n >= NS) of hypothesis h of pair (k, l): a counter-based generator, rejection of repeats;
// the first draws do not depend on NS (8 for the fundamental matrix; 6, with l = k, for a camera matrix: mvba_resect_ransac.h).
// Every index of idx is a compile-time constant once the loops are unrolled (registers on the device).
template <int NS>
__host__ __device__ __forceinline__ void rs_sample(unsigned long long seed, int k, int l, int h, long long n, long long (&idx)[NS]) {
  unsigned long long s = rs_mix(rs_mix(rs_mix(seed) ^ (((unsigned long long)(unsigned int)k << 32) | (unsigned long long)(unsigned int)l)) ^
                                (unsigned long long)(unsigned int)h);
#pragma unroll
  for (int c = 0; c < NS; ++c) {
    long long j;
    bool dup;
    do {
      s = rs_mix(s);
      j = (long long)(((s >> 32) * (unsigned long long)n) >> 32);  // (n < 2^31: the product is below 2^63)
      dup = false;
#pragma unroll
      for (int e = 0; e < NS; ++e)
        if (e < c && idx[e] == j) dup = true;
    } while (dup);
    idx[c] = j;
  }
}

// The body of the *_sample entry points that rs_sample serves: the NS indices of hypothesis h of item (k, l) among n, for a
// test to draw what the kernels draw.  `keys` names the indices the entry point takes ("klh", "kh", "h"), for its message; out
// is its argument number `arg`, called `name`.
template <int NS>
int sample_entry(uint64_t seed, const char *keys, int32_t k, int32_t l, int32_t h, int64_t n, int64_t *out, const char *name, int arg) {
  if (!out) return fail(MVBA_ERR_BADARG, std::string("null argument: ") + name + " (argument " + std::to_string(arg) + ")");
  if (n < NS || n >= (1LL << 31)) return fail(MVBA_ERR_BADARG, "n = " + std::to_string(n) + " must be in " + std::to_string(NS) + " .. 2^31 - 1");
  if (k < 0 || l < 0 || h < 0) {
    std::string msg;
    for (const char *c = keys; *c; ++c)
      msg += std::string(c == keys ? "" : ", ") + *c + " = " + std::to_string(*c == 'k' ? k : (*c == 'l' ? l : h));
    return fail(MVBA_ERR_BADARG, msg + ": negative index");
  }
  long long idx[NS];
  rs_sample(seed, k, l, h, n, idx);
  for (int c = 0; c < NS; ++c) out[c] = idx[c];
  return MVBA_OK;
}

// cnt[pair][chunk] = the number of shared points among the chunk's 256
__global__ __launch_bounds__(START_CHUNK) void k_ransac_count(long long npts, int m, const long long *__restrict__ pt_ptr,
                                                           const int *__restrict__ cam_idx, const int *__restrict__ pairs,
                                                           int *__restrict__ cnt) {
  __shared__ int s_w[START_CHUNK / 64];
  const int p = blockIdx.y, i = threadIdx.x;
  long long ok, ol;
  const bool sh = rs_shared((long long)blockIdx.x * START_CHUNK + i, npts, m, pt_ptr, cam_idx, pairs[2 * p], pairs[2 * p + 1], ok, ol);
  chunk_ballot(sh, s_w);
  if (i == 0) cnt[(size_t)p * gridDim.x + blockIdx.x] = chunk_total(s_w);
}

// one workgroup per pair: cnt[pair][.] -> its exclusive prefix sums, in place; ntot[pair] = the total.  Thread i takes a
// contiguous run of chunks; thread 0 scans the 256 run sums.
__global__ __launch_bounds__(256) void k_ransac_scan(int n_ch, int *__restrict__ cnt, int *__restrict__ ntot) {
  __shared__ int s[256];
  const int p = blockIdx.x, i = threadIdx.x;
  int *c = cnt + (size_t)p * n_ch;
  const int per = (n_ch + 255) / 256, a = min(n_ch, i * per), b = min(n_ch, a + per);
  int sum = 0;
  for (int e = a; e < b; ++e) sum += c[e];
  s[i] = sum;
  __syncthreads();
  if (i == 0) {
    int run = 0;
    for (int t = 0; t < 256; ++t) {
      const int v = s[t];
      s[t] = run;
      run += v;
    }
    ntot[p] = run;
  }
  __syncthreads();
  int run = s[i];
  for (int e = a; e < b; ++e) {
    const int v = c[e];
    c[e] = run;
    run += v;
  }
}

// comp[pair][j] = (x_k, y_k, x_l, y_l) and id[pair][j] = the point of the pair's j-th shared point, ascending
__global__ __launch_bounds__(START_CHUNK) void k_ransac_compact(long long npts, int m, const long long *__restrict__ pt_ptr,
                                                             const int *__restrict__ cam_idx, const double2 *__restrict__ xy,
                                                             const int *__restrict__ pairs, const int *__restrict__ off,
                                                             double4 *__restrict__ comp, int *__restrict__ id) {
  __shared__ int s_w[START_CHUNK / 64];
  const int p = blockIdx.y, i = threadIdx.x;
  const long long a = (long long)blockIdx.x * START_CHUNK + i;
  long long ok, ol;
  const bool sh = rs_shared(a, npts, m, pt_ptr, cam_idx, pairs[2 * p], pairs[2 * p + 1], ok, ol);
  const unsigned long long b = chunk_ballot(sh, s_w);
  if (!sh) return;
  const int j = off[(size_t)p * gridDim.x + blockIdx.x] + chunk_rank(b, s_w);
  const double2 zk = xy[ok], zl = xy[ol];
  comp[(size_t)p * npts + j] = make_double4(zk.x, zk.y, zl.x, zl.y);  // (j < the pair's count <= npts)
  id[(size_t)p * npts + j] = (int)a;
}

// The passes 0, 1, 2 of k_twoview_chunk (tv_pass, chunk_sum) over the compacted array: part[pair][chunk][NV] over the points j < ntot[pair] whose
// byte in the pair's current mask is set (state == nullptr: every point).  A pair that is not RS_ACTIVE sums nothing.
template <int MODE>
__global__ __launch_bounds__(START_CHUNK) void k_ransac_fit(long long stride, const int *__restrict__ ntot, const int *__restrict__ state,
                                                         const double4 *__restrict__ comp, const unsigned char *__restrict__ inl0,
                                                         const unsigned char *__restrict__ inl1, const double *__restrict__ aux,
                                                         double *__restrict__ part) {
  constexpr int NV = tv_values(MODE);
  __shared__ double s_w[START_CHUNK / 64][NV];
  const int p = blockIdx.y, i = threadIdx.x;
  const long long j = (long long)blockIdx.x * START_CHUNK + i;
  double v[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) v[e] = 0.0;
  bool use = j < ntot[p];
  if (state) {
    const int st = state[p];
    use = use && (st & RS_ACTIVE);
    if (use) use = rs_current(st, inl0, inl1)[(size_t)p * stride + j] != 0;
  }
  if (use) {
    const double4 z = comp[(size_t)p * stride + j];
    tv_pass<MODE>(z.x, z.y, z.z, z.w, aux + tv_aux(MODE) * (size_t)p, v);
  }
  chunk_sum<NV>(v, s_w, part + ((size_t)p * gridDim.x + blockIdx.x) * NV);
}

// One thread per hypothesis: sample, M = sum of a a^T over the 8 normalised rows, cyclic Jacobi in LDS, F^ = the eigenvector
// of the smallest eigenvalue -> hypf, F = T_l^T F^ T_k -> hypF; hyp_count = 0, or -1 (and NaN matrices) if degenerate.
__global__ __launch_bounds__(RS_HYP_BLOCK) void k_ransac_hyp(long long stride, int H, unsigned long long seed, const int *__restrict__ pairs,
                                                             const int *__restrict__ ntot, const double4 *__restrict__ comp,
                                                             const double *__restrict__ norm, double *__restrict__ hypf,
                                                             double *__restrict__ hypF, int *__restrict__ hyp_count) {
  extern __shared__ double s_rs[];  // A [81][64], V [81][64]
  const int p = blockIdx.y, tid = threadIdx.x, h = blockIdx.x * RS_HYP_BLOCK + tid;
  if (h >= H) return;  // (no barrier below: a thread works on its own LDS column)
  const size_t o9 = ((size_t)p * H + h) * 9;
  const int n = ntot[p];
  bool good = n >= TV_MIN_SHARED;  // (below 8 the rejection loop of rs_sample would not end)
  double fh[9], F[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) fh[e] = F[e] = NAN;
  if (good) {
    double *sA = s_rs + tid, *sV = s_rs + 81 * RS_HYP_BLOCK + tid;
    auto A = [&](int r, int c) -> double & { return sA[(r * 9 + c) * RS_HYP_BLOCK]; };
    const double *nm = norm + TV_NORM * (size_t)p;
    long long idx[8];
    rs_sample(seed, pairs[2 * p], pairs[2 * p + 1], h, n, idx);
    double M[45];
#pragma unroll
    for (int e = 0; e < 45; ++e) M[e] = 0.0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const double4 z = comp[(size_t)p * stride + idx[c]];
      double r[9];
      tv_row(nm, z.x, z.y, z.z, z.w, r);
      int e = 0;
#pragma unroll
      for (int b = 0; b < 9; ++b)
#pragma unroll
        for (int d = b; d < 9; ++d, ++e) M[e] += r[b] * r[d];
    }
    {
      int e = 0;
#pragma unroll
      for (int b = 0; b < 9; ++b)
#pragma unroll
        for (int d = b; d < 9; ++d, ++e) {
          good = good && isfinite(M[e]);
          A(b, d) = M[e];
          A(d, b) = M[e];
        }
    }
    good = rs_lds_eig<9>(sA, sV, good, fh);
    if (good) {
      tv_denormalise(nm, fh, F);  // (no rank-2 step: a hypothesis is scored as the sample gives it)
#pragma unroll
      for (int e = 0; e < 9; ++e) good = good && isfinite(F[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    hypf[o9 + e] = good ? fh[e] : NAN;
    hypF[o9 + e] = good ? F[e] : NAN;
  }
  hyp_count[(size_t)p * H + h] = good ? 0 : -1;
}

// What the scoring and mask kernels test a point against: PARTS 3 x 3 matrices per hypothesis (part a of pair p of a tile of
// cnt pairs at [(a cnt + p) ...]: the parts are whole arrays, one behind the other), the fewest points MIN a pair needs, and
// inlier, the test the scoring kernel counts by, and dist2, the squared distance the mask pass sums and tests: a point is an
// inlier there if it is <= threshold^2, and the two agree on every point (a model with a test of its own returns infinity from
// dist2 where that fails).  The fundamental matrix: one part, the Sampson distance.  (The homography: mvba_homography.h.)
struct FundModel {
  static constexpr int PARTS = 1, MIN = TV_MIN_SHARED;
  static __device__ __forceinline__ double dist2(const double *F, const double *, double xk, double yk, double xl, double yl, double) {
    return rs_sampson(F, xk, yk, xl, yl);
  }
  static __device__ __forceinline__ bool inlier(const double *F, const double *, double xk, double yk, double xl, double yl, double thr2) {
    return rs_sampson(F, xk, yk, xl, yl) <= thr2;
  }
};

// Scoring: grid (chunks of compacted points, blocks of 64 hypotheses, pairs).  A thread holds one point and walks the block's
// matrices in LDS (every lane reads the same address: a broadcast); a hypothesis's inliers of a wave are one ballot and one
// popcount, kept by the lane of the hypothesis's number; then integer atomics.  A degenerate hypothesis is NaN: no point
// passes, its count stays -1.
template <class M>
__global__ __launch_bounds__(START_CHUNK) void k_ransac_score(long long stride, int H, const int *__restrict__ ntot,
                                                           const double4 *__restrict__ comp, const double *__restrict__ hypF,
                                                           double thr2, int *__restrict__ hyp_count) {
  __shared__ double s_F[M::PARTS][RS_HYP_BLOCK * 9];
  __shared__ int s_cnt[RS_HYP_BLOCK];
  const int p = blockIdx.z, h0 = blockIdx.y * RS_HYP_BLOCK, i = threadIdx.x, lane = i & 63;
  const int n = ntot[p];
  const long long j = (long long)blockIdx.x * START_CHUNK + i;
  if (n < M::MIN || (long long)blockIdx.x * START_CHUNK >= n) return;  // (the whole workgroup leaves)
  const int nh = min(RS_HYP_BLOCK, H - h0);
  for (int e = i; e < nh * 9; e += START_CHUNK) s_F[0][e] = hypF[((size_t)p * H + h0) * 9 + e];
  if constexpr (M::PARTS == 2)
    for (int e = i; e < nh * 9; e += START_CHUNK) s_F[1][e] = hypF[(((size_t)gridDim.z + p) * H + h0) * 9 + e];
  if (i < RS_HYP_BLOCK) s_cnt[i] = 0;
  __syncthreads();
  const bool live = j < n;
  const double4 z = live ? comp[(size_t)p * stride + j] : make_double4(0.0, 0.0, 0.0, 0.0);
  const int mine = rs_score_block(nh, lane, live, [&](int hh) {
    return M::inlier(s_F[0] + 9 * hh, s_F[M::PARTS - 1] + 9 * hh, z.x, z.y, z.z, z.w, thr2);
  });
  rs_score_add(mine, nh, lane, s_cnt, hyp_count + (size_t)p * H + h0);
}

// Fcur[pair], fbest[pair] = the matrices of the pair's best hypothesis (best < 0: NaN)
__global__ __launch_bounds__(256) void k_ransac_gather(int n_pairs, int H, const int *__restrict__ best, const double *__restrict__ hypF,
                                                       const double *__restrict__ hypf, double *__restrict__ Fcur, double *__restrict__ fbest) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_pairs * 9) return;
  const int p = t / 9, e = t - 9 * p, b = best[p];
  Fcur[t] = b >= 0 ? hypF[((size_t)p * H + b) * 9 + e] : NAN;
  fbest[t] = b >= 0 ? hypf[((size_t)p * H + b) * 9 + e] : NAN;
}

// The inlier set of the pair's matrices F[part][pair] into the pair's OTHER mask buffer, and part[pair][chunk][2] = (count, sum of d^2 over it) by the
// tree of chunk_sum (the count is exact in a double).  A pair that is not RS_ACTIVE writes nothing and sums nothing.
template <class M>
__global__ __launch_bounds__(START_CHUNK) void k_ransac_mask(long long stride, const int *__restrict__ ntot, const int *__restrict__ state,
                                                          const double4 *__restrict__ comp, const double *__restrict__ F, double thr2,
                                                          unsigned char *__restrict__ inl0, unsigned char *__restrict__ inl1,
                                                          double *__restrict__ part) {
  __shared__ double s_w[START_CHUNK / 64][2];
  const int p = blockIdx.y, i = threadIdx.x, st = state[p];
  const long long j = (long long)blockIdx.x * START_CHUNK + i;
  double v[2] = {0.0, 0.0};
  if ((st & RS_ACTIVE) && j < ntot[p]) {
    const double4 z = comp[(size_t)p * stride + j];
    const double *F0 = F + 9 * (size_t)p;
    const double d2 = M::dist2(F0, F0 + (size_t)(M::PARTS - 1) * gridDim.y * 9, z.x, z.y, z.z, z.w, thr2);
    mask_step(d2 <= thr2, d2, &rs_other(st, inl0, inl1)[(size_t)p * stride + j], v);
  }
  chunk_sum<2>(v, s_w, part + ((size_t)p * gridDim.x + blockIdx.x) * 2);
}

// out[pair][point] = 1 for the points of the pair's current mask (pairs of status 0; out is zero beforehand)
__global__ __launch_bounds__(START_CHUNK) void k_ransac_scatter(long long stride, const int *__restrict__ ntot, const int *__restrict__ state,
                                                             const int *__restrict__ id, const unsigned char *__restrict__ inl0,
                                                             const unsigned char *__restrict__ inl1, unsigned char *__restrict__ out) {
  const int p = blockIdx.y, st = state[p];
  const long long j = (long long)blockIdx.x * START_CHUNK + threadIdx.x;
  if (!(st & RS_OK) || j >= ntot[p]) return;
  if (rs_current(st, inl0, inl1)[(size_t)p * stride + j]) out[(size_t)p * stride + id[(size_t)p * stride + j]] = 1;
}

// F^ (unit, normalised units) -> F through twoview_solve_pair's own rank-2 step, denormalisation and scaling: the moment
// matrix I - f f^T has f as the eigenvector of its one zero eigenvalue (the others are 1).
int ransac_finish_hypothesis(const double *fh, const double *nm, double *F) {
  double S45[45], ratio;
  int e = 0;
  for (int b = 0; b < 9; ++b)
    for (int c = b; c < 9; ++c, ++e) S45[e] = (b == c ? 1.0 : 0.0) - fh[b] * fh[c];
  return twoview_solve_pair(S45, nm, F, &ratio);
}

// The model-specific steps of robust_pairs, for the fundamental matrix: the hypothesis kernel (F in part 0, F^ in part 1 of
// hyp), the refit's moments (tv_pass mode 2) and eigen-solve, and what a hypothesis that no refit replaces becomes.
struct FundFit {
  using Model = FundModel;
  static constexpr int MOMENTS = 2;
  static constexpr size_t HYP_BYTES = RS_HYP_BYTES;
  static constexpr const char *NAME = "F";
  static constexpr int hyp_lds = (int)(sizeof(double) * 2 * 81 * RS_HYP_BLOCK);
  static int prepare() {
    MVBA_HIP(hipFuncSetAttribute((const void *)k_ransac_hyp, hipFuncAttributeMaxDynamicSharedMemorySize, hyp_lds));
    return MVBA_OK;
  }
  static void hypotheses(int cnt, long long stride, int H, unsigned long long seed, const int *pairs, const int *ntot, const double4 *comp,
                         const double *norm, double *hyp, int *hyp_count) {
    hipLaunchKernelGGL(k_ransac_hyp, dim3((H + RS_HYP_BLOCK - 1) / RS_HYP_BLOCK, cnt), dim3(RS_HYP_BLOCK), hyp_lds, 0, stride, H, seed, pairs, ntot,
                       comp, norm, hyp + 9 * (size_t)cnt * H, hyp, hyp_count);
  }
  // the pair's best hypothesis (part 0 and part 1 of it) -> the matrix the call returns if no refit is kept
  static int finish(const double *, const double *fh, const double *nm, double *F) { return ransac_finish_hypothesis(fh, nm, F); }
  static int solve(const double *S45, const double *nm, double *F, double *ratio) { return twoview_solve_pair(S45, nm, F, ratio); }
  // a refit's matrix -> the parts the mask kernel tests against
  static void mask_parts(const double *F, const double *, double *m0, double *) { std::copy(F, F + 9, m0); }
};

// The pair-tile loop of a robust two-view fit, once: mvba_two_view_robust (FundFit) and mvba_homography_robust (HomogFit,
// mvba_homography.h) are this function.  `F` is the model's matrix, whatever it is called.
template <class Fit>
int robust_pairs(int64_t n_points, int32_t n_images, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy, int64_t n_obs,
                 const int32_t *pairs, int32_t n_pairs, double threshold, int32_t n_hypotheses, uint64_t seed, int32_t n_refit,
                 double *F, double *quality, int64_t *n_shared, int64_t *n_inliers, int32_t *best, uint8_t *inlier,
                 int32_t *hyp_count, int32_t *status, double *timings_ms, int32_t device) {
  using Model = typename Fit::Model;
  if (n_pairs < 0) return fail(MVBA_ERR_BADARG, "n_pairs = " + std::to_string(n_pairs) + " must be >= 0");
  if (!xy || (n_pairs > 0 && (!pairs || !F)))
    return fail(MVBA_ERR_BADARG, std::string("null argument: ") + (!xy ? "xy" : (!pairs ? "pairs" : Fit::NAME)) + " (argument " +
                                     std::to_string(!xy ? 5 : (!pairs ? 7 : 13)) + ")");
  int rc;
  if ((rc = rs_check_search(threshold, n_hypotheses)) || (rc = rs_check_refit(n_refit))) return rc;
  if ((rc = init_check_list(n_points, n_images, pt_ptr, cam_idx, n_obs))) return rc;
  if ((rc = init_check_cameras(n_images))) return rc;
  if ((rc = check_pairs(pairs, n_pairs, n_images))) return rc;
  if ((rc = check_ascending(n_points, pt_ptr, cam_idx))) return rc;
  if (timings_ms) timings_ms[0] = timings_ms[1] = timings_ms[2] = timings_ms[3] = 0.0;
  const int np = n_pairs, H = n_hypotheses;
  const double thr2 = threshold * threshold;
  // the defaults are those of a pair without shared points: status 1
  if (np > 0) std::fill(F, F + 9 * (size_t)np, NAN);
  RsTile::defaults((size_t)np, H, status, best, hyp_count, n_shared, n_inliers, quality);
  if (inlier) std::memset(inlier, 0, (size_t)np * (size_t)n_points);
  if (np == 0 || n_points == 0) return MVBA_OK;

  if (device >= 0) MVBA_HIP(hipSetDevice(device));
  InitClock clk;
  const long long n_ch = (n_points + START_CHUNK - 1) / START_CHUNK;
  const long long stride = n_points;
  const int tile = tv_pair_tile(np, RS_POINT_BYTES * (size_t)n_points + Fit::HYP_BYTES * (size_t)H);
  DevBufs tmp;
  double2 *dxy = nullptr;
  long long *dptr = nullptr;
  int *dcam = nullptr, *dpairs = nullptr, *doff = nullptr, *dntot = nullptr, *did = nullptr, *dstate = nullptr, *dbest = nullptr, *dhc = nullptr;
  double4 *dcomp = nullptr;
  unsigned char *dinl0 = nullptr, *dinl1 = nullptr, *dout = nullptr;
  double *dpart = nullptr, *dS = nullptr, *dnorm = nullptr, *dnorm2 = nullptr, *dF = nullptr, *dhyp = nullptr;
  const size_t ts = (size_t)tile * (size_t)stride;
  if ((rc = upload_list(tmp, n_points, n_obs, pt_ptr, cam_idx, xy, &dptr, &dcam, &dxy)) || (rc = tmp.alloc(&dpairs, 2 * (size_t)np)) || (rc = tmp.alloc(&doff, (size_t)tile * n_ch)) ||
      (rc = tmp.alloc(&dntot, (size_t)tile)) || (rc = tmp.alloc(&did, ts)) || (rc = tmp.alloc(&dstate, (size_t)tile)) ||
      (rc = tmp.alloc(&dbest, (size_t)tile)) || (rc = tmp.alloc(&dhc, (size_t)tile * H)) || (rc = tmp.alloc(&dcomp, ts)) ||
      (rc = tmp.alloc(&dinl0, ts)) || (rc = tmp.alloc(&dinl1, ts)) || (rc = tmp.alloc(&dpart, 45 * (size_t)n_ch * tile)) ||
      (rc = tmp.alloc(&dS, 45 * (size_t)tile)) || (rc = tmp.alloc(&dnorm, TV_NORM * (size_t)tile)) || (rc = tmp.alloc(&dnorm2, TV_NORM * (size_t)tile)) ||
      (rc = tmp.alloc(&dF, 18 * (size_t)tile)) || (rc = tmp.alloc(&dhyp, 18 * (size_t)tile * H)))
    return rc;
  if (inlier && (rc = tmp.alloc(&dout, ts))) return rc;
  MVBA_HIP(hipMemcpy(dpairs, pairs, sizeof(int) * 2 * np, hipMemcpyHostToDevice));
  if ((rc = Fit::prepare())) return rc;
  RsLaps laps;
  laps.upload = clk.lap();

  const dim3 b256(256), bch(START_CHUNK);
  std::vector<int> ntot((size_t)tile), hc((size_t)tile * H), state((size_t)tile);
  RsTile t(tile);
  std::vector<double> S((size_t)tile * 45), norm(TV_NORM * (size_t)tile), fb(18 * (size_t)tile), Fc(9 * (size_t)tile), Fn(9 * (size_t)tile), Mn(18 * (size_t)tile),
      S2(2 * (size_t)tile), ratio((size_t)tile);
  for (int p0 = 0; p0 < np; p0 += tile) {
    const int cnt = std::min(tile, np - p0);
    const dim3 grid((unsigned)n_ch, (unsigned)cnt), gp((cnt + 255) / 256);
    const int *tp = dpairs + 2 * (size_t)p0;
    auto combine = [&](int nv, double *out) { tv_combine(cnt, nv, n_ch, dpart, out, nv); };
    // the normalised moment sums of the pairs' current masks (st_dev == nullptr: of all shared points, passes 0 and 1 only)
    auto fit = [&](const int *st_dev, double *nm_dev, bool moments) {
      hipLaunchKernelGGL(k_ransac_fit<0>, grid, bch, 0, 0, stride, dntot, st_dev, dcomp, dinl0, dinl1, (const double *)nullptr, dpart);
      combine(5, dS);
      hipLaunchKernelGGL(k_twoview_norm, gp, b256, 0, 0, cnt, 0, dS, 5, nm_dev);
      hipLaunchKernelGGL(k_ransac_fit<1>, grid, bch, 0, 0, stride, dntot, st_dev, dcomp, dinl0, dinl1, nm_dev, dpart);
      combine(2, dS);
      hipLaunchKernelGGL(k_twoview_norm, gp, b256, 0, 0, cnt, 1, dS, 2, nm_dev);
      if (moments) {
        hipLaunchKernelGGL(k_ransac_fit<Fit::MOMENTS>, grid, bch, 0, 0, stride, dntot, st_dev, dcomp, dinl0, dinl1, nm_dev, dpart);
        combine(45, dS);
      }
    };
    // the inlier sets of dF under the pairs' states: counts and sums of d^2 into S2
    auto mask = [&]() -> int {
      MVBA_HIP(hipMemcpy(dstate, state.data(), sizeof(int) * cnt, hipMemcpyHostToDevice));
      hipLaunchKernelGGL(k_ransac_mask<Model>, grid, bch, 0, 0, stride, dntot, dstate, dcomp, dF, thr2, dinl0, dinl1, dpart);
      combine(2, dS);
      MVBA_HIP(hipGetLastError());
      MVBA_HIP(hipMemcpy(S2.data(), dS, sizeof(double) * 2 * cnt, hipMemcpyDeviceToHost));
      return MVBA_OK;
    };

    // compaction, normalisation over all shared points, hypotheses, scores
    hipLaunchKernelGGL(k_ransac_count, grid, bch, 0, 0, (long long)n_points, n_images, dptr, dcam, tp, doff);
    hipLaunchKernelGGL(k_ransac_scan, dim3(cnt), b256, 0, 0, (int)n_ch, doff, dntot);
    hipLaunchKernelGGL(k_ransac_compact, grid, bch, 0, 0, (long long)n_points, n_images, dptr, dcam, dxy, tp, doff, dcomp, did);
    fit(nullptr, dnorm, false);
    Fit::hypotheses(cnt, stride, H, (unsigned long long)seed, tp, dntot, dcomp, dnorm, dhyp, dhc);
    hipLaunchKernelGGL(k_ransac_score<Model>, dim3((unsigned)n_ch, (H + RS_HYP_BLOCK - 1) / RS_HYP_BLOCK, cnt), bch, 0, 0, stride, H, dntot, dcomp,
                       dhyp, thr2, dhc);
    MVBA_HIP(hipGetLastError());
    MVBA_HIP(hipMemcpy(hc.data(), dhc, sizeof(int) * (size_t)cnt * H, hipMemcpyDeviceToHost));
    MVBA_HIP(hipMemcpy(ntot.data(), dntot, sizeof(int) * cnt, hipMemcpyDeviceToHost));
    MVBA_HIP(hipMemcpy(norm.data(), dnorm, sizeof(double) * TV_NORM * cnt, hipMemcpyDeviceToHost));
    laps.score += clk.lap();

    t.pick(cnt, state.data(), hc.data(), H, ntot.data(), Model::MIN);
    MVBA_HIP(hipMemcpy(dbest, t.best.data(), sizeof(int) * cnt, hipMemcpyHostToDevice));
    // the two parts of the best hypothesis, one array behind the other: what the mask kernel reads
    hipLaunchKernelGGL(k_ransac_gather, dim3((cnt * 9 + 255) / 256), b256, 0, 0, cnt, H, dbest, dhyp, dhyp + 9 * (size_t)cnt * H, dF, dF + 9 * (size_t)cnt);
    if ((rc = mask())) return rc;
    MVBA_HIP(hipMemcpy(fb.data(), dF, sizeof(double) * 18 * cnt, hipMemcpyDeviceToHost));
    t.first(S2.data(), [&](int p) {
      ratio[p] = 0.0;  // (the moment matrix of a minimal sample has rank 8)
      return Fit::finish(fb.data() + 9 * (size_t)p, fb.data() + 9 * (size_t)(cnt + p), norm.data() + TV_NORM * (size_t)p, Fc.data() + 9 * (size_t)p);
    });
    laps.other += clk.lap();

    // refits: the full fit on the current inliers alone, kept while its own inlier set does not shrink
    for (int r = 0; r < n_refit && t.n_active > 0; ++r) {
      MVBA_HIP(hipMemcpy(dstate, state.data(), sizeof(int) * cnt, hipMemcpyHostToDevice));
      fit(dstate, dnorm2, true);
      MVBA_HIP(hipGetLastError());
      MVBA_HIP(hipMemcpy(S.data(), dS, sizeof(double) * 45 * cnt, hipMemcpyDeviceToHost));
      MVBA_HIP(hipMemcpy(norm.data(), dnorm2, sizeof(double) * TV_NORM * cnt, hipMemcpyDeviceToHost));
      std::vector<double> rt((size_t)cnt, NAN);
      for (int p = 0; p < cnt; ++p) {
        for (int j = 0; j < 9; ++j) Fn[9 * (size_t)p + j] = Mn[9 * (size_t)p + j] = Mn[9 * (size_t)(cnt + p) + j] = NAN;
        if (!(state[p] & RS_ACTIVE)) continue;
        const double *nm = norm.data() + TV_NORM * (size_t)p;
        if (Fit::solve(S.data() + 45 * (size_t)p, nm, Fn.data() + 9 * (size_t)p, &rt[p])) rs_stop(state[p], t.n_active);
        else Fit::mask_parts(Fn.data() + 9 * (size_t)p, nm, Mn.data() + 9 * (size_t)p, Mn.data() + 9 * (size_t)(cnt + p));
      }
      if (t.n_active == 0) break;
      MVBA_HIP(hipMemcpy(dF, Mn.data(), sizeof(double) * 9 * Model::PARTS * cnt, hipMemcpyHostToDevice));
      if ((rc = mask())) return rc;
      t.accept(r, S2.data(), 0, [&](int p) {
        ratio[p] = rt[p];
        for (int j = 0; j < 9; ++j) Fc[9 * (size_t)p + j] = Fn[9 * (size_t)p + j];
      });
    }
    laps.refit += clk.lap();

    if (inlier) {
      MVBA_HIP(hipMemcpy(dstate, state.data(), sizeof(int) * cnt, hipMemcpyHostToDevice));
      MVBA_HIP(hipMemset(dout, 0, (size_t)cnt * stride));
      hipLaunchKernelGGL(k_ransac_scatter, grid, bch, 0, 0, stride, dntot, dstate, did, dinl0, dinl1, dout);
      MVBA_HIP(hipGetLastError());
      MVBA_HIP(hipMemcpy(inlier + (size_t)p0 * stride, dout, (size_t)cnt * stride, hipMemcpyDeviceToHost));
    }
    if (n_shared) std::copy(ntot.begin(), ntot.begin() + cnt, n_shared + p0);
    t.write((size_t)p0, status, best, hyp_count, n_inliers, quality, [&](int p) {
      for (int j = 0; j < 9; ++j) F[9 * ((size_t)p0 + p) + j] = Fc[9 * (size_t)p + j];
      return ratio[p];
    });
    laps.other += clk.lap();
  }
  laps.write(timings_ms);
  return MVBA_OK;
}

}  // namespace

extern "C" {

int mvba_ransac_sample(uint64_t seed, int32_t k, int32_t l, int32_t h, int64_t n, int64_t *idx8) {
  return sample_entry<TV_MIN_SHARED>(seed, "klh", k, l, h, n, idx8, "idx8", 6);
}

int mvba_two_view_robust(int64_t n_points, int32_t n_images, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy, int64_t n_obs,
                         const int32_t *pairs, int32_t n_pairs, double threshold, int32_t n_hypotheses, uint64_t seed, int32_t n_refit,
                         double *F, double *quality, int64_t *n_shared, int64_t *n_inliers, int32_t *best, uint8_t *inlier,
                         int32_t *hyp_count, int32_t *status, double *timings_ms, int32_t device) {
  return robust_pairs<FundFit>(n_points, n_images, pt_ptr, cam_idx, xy, n_obs, pairs, n_pairs, threshold, n_hypotheses, seed, n_refit, F, quality,
                               n_shared, n_inliers, best, inlier, hyp_count, status, timings_ms, device);
}

}  // extern "C"
