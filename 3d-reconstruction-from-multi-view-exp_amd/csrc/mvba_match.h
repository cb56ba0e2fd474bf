// Matching of uint8 descriptors (mvba_match_descriptors) -- kernels and host code, gfx950.
//
// Included by mvba.hip after mvba_tracks.h: uses its tracks_scan, trk_grid and trk_u64, mvba_start.h's InitClock and EvGuard,
// mvba.hip's DevBufs, fail and MVBA_HIP, and mvba_match_host.h's checks, chunk rule and ratio test.  Nothing here runs on the
// LM path.  
//
// Integers only, except the one double multiply and compare of the ratio test; no atomics.  A byte x becomes the signed byte
// x - 128 by x ^ 0x80 (whole dwords at a time), which leaves every distance as it is, and
//   d2(a, b) = |a'|^2 + |b'|^2 - 2 a'.b'
// with the dot products from v_mfma_i32_32x32x32_i8 and the squared norms from k_match_norm.  dim <= 512 keeps every term and
// every sum of them inside i32.
//
// Orientation.  The candidates are the A operand, staged through LDS in tiles of MATCH_TC rows and shared by the workgroup's
// four waves; the queries are the B operand, 32 per wave, their fragments loaded once and held in registers.  The C/D map of
// the instruction puts the column on the lane (lane & 31) and 16 rows in its registers (row = (reg & 3) + 8 (reg >> 2) +
// 4 (lane >> 5)): a lane owns ONE query for the whole sweep and sees 16 candidates of it per MFMA tile, in ascending order of
// the candidate index.  So the running nearest two (and the index of the nearest) live in the lane's registers, a strict
// `<` keeps the smaller index on a tie, and the only cross-lane step is the merge of lane and lane ^ 32 at the end.  Both
// operands are loaded with the same lane-to-k map (lane half h takes bytes 16 h .. 16 h + 15 of a k step), so whatever
// permutation of k the instruction applies inside a step cancels in the dot product.
//
// A directed job is (query image, candidate image); a workgroup owns MATCH_TQ queries of one job and sweeps all its candidate
// tiles.  The reverse direction of the mutual check is a second list of jobs (best only).  One thread per query then applies
// rules 1 to 4; an integer scan (tracks_scan) compacts the matches; the per-rule counts leave each workgroup as partial sums
// that the host adds.

namespace {

typedef int match_v4 __attribute__((ext_vector_type(4)));
typedef int match_v16 __attribute__((ext_vector_type(16)));

constexpr int MATCH_NONE = 0x7fffffff;      // "no distance yet"
constexpr int MATCH_PAD_KEY = -(1 << 30);   // the key of a row beyond the image: v = MATCH_PAD_V, above every |b'|^2 - 2 a'.b' (below 2^25 in magnitude)
constexpr int MATCH_PAD_V = 1 << 26;
constexpr unsigned MATCH_FLIP = 0x80808080u;  // x ^ 0x80 on the four bytes of a dword: x - 128 as a signed byte

// MATCH_TQ queries [q0, q0 + nq) (node ids) of one directed job against the candidates [c0, c0 + nc); results at out0 + local query
struct MatchBlock {
  int q0, nq, c0, nc, out0;
};

__device__ __forceinline__ match_v4 match_load16(const unsigned char *p) {
  const uint4 v = *reinterpret_cast<const uint4 *>(p);
  match_v4 r;
  r.x = (int)(v.x ^ MATCH_FLIP);
  r.y = (int)(v.y ^ MATCH_FLIP);
  r.z = (int)(v.z ^ MATCH_FLIP);
  r.w = (int)(v.w ^ MATCH_FLIP);
  return r;
}

__device__ __forceinline__ int match_dot4(int acc, int w) {  // the four signed bytes of w, squared and summed
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int b = (w << (24 - 8 * e)) >> 24;
    acc += b * b;
  }
  return acc;
}

// norm2[v] = |desc[v] - 128|^2, one thread per node
__global__ __launch_bounds__(256) void k_match_norm(int n, int dim, const unsigned char *__restrict__ desc, int *__restrict__ norm2) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const unsigned char *row = desc + (size_t)v * dim;
  int s = 0;
  for (int k = 0; k < dim; k += 16) {
    const match_v4 w = match_load16(row + k);
    s = match_dot4(match_dot4(match_dot4(match_dot4(s, w.x), w.y), w.z), w.w);
  }
  norm2[v] = s;
}

// The nearest (SECOND: nearest two) candidates of every query of a list of blocks.  KS: the k steps of a descriptor, a power of
// two (32 KS >= dim; the bytes beyond dim are zeros after the shift, in LDS and in the query fragments alike).  Dynamic LDS:
// match_nn_lds(KS).  best: the candidate's index local to its image (-1: none), best2 its squared distance (-1: none), second2
// that of the second (-1: none).
//
// The update.  With v = |b'|^2 - 2 a'.b' (the query's own norm moves no argmin and is added at the end), a tile's element is
// reduced as the KEY  K = (dot << 5) + key[row],  key[row] = -16 |b'|^2 + 15 - reg(row)  from the staging pass: K = -16 v + (15 -
// reg), one v_lshl_add per element.  A larger K is a smaller v, and among equal v the smaller register, which is the smaller
// candidate index (rows ascend with reg).  So per element: t2 = med3(K, t1, t2); t1 = max(K, t1).  |v| < 2^25 at dim = 512, so K
// stays inside i32.  Once per tile the lane unpacks (v = -(t >> 4), reg = 15 - (t & 15)) and merges the tile's two with its
// running two by v alone, a strict `<`: the earlier tile keeps a tie.  A row beyond the image has key -2^30, v = 2^26.
template <int KS, bool SECOND>
__global__ __launch_bounds__(256) void k_match_nn(const MatchBlock *__restrict__ blocks, const unsigned char *__restrict__ desc, int dim,
                                                  const int *__restrict__ norm2, int *__restrict__ best, int *__restrict__ best2,
                                                  int *__restrict__ second2) {
  extern __shared__ __align__(16) unsigned char s_match[];
  constexpr int per_row = 2 * KS, stride = MATCH_KSTEP * KS + 16;  // 16-byte pieces of a row; its bytes, with 16 of padding
  int *s_key = reinterpret_cast<int *>(s_match);              // [MATCH_TC]
  unsigned char *s_cand = s_match + sizeof(int) * MATCH_TC;   // [MATCH_TC][stride]
  const MatchBlock B = blocks[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int ql = wave * 32 + r;           // this lane's query, local to the block
  const bool wave_on = wave * 32 < B.nq;  // (uniform per wave)

  match_v4 qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k0 = MATCH_KSTEP * s + 16 * h;
    qf[s] = match_v4{0, 0, 0, 0};  // beyond dim, and beyond the block's queries: zeros AFTER the shift
    if (ql < B.nq && k0 < dim) qf[s] = match_load16(desc + (size_t)(B.q0 + ql) * dim + k0);
  }

  int b1 = MATCH_NONE, b2 = MATCH_NONE, i1 = -1;
  for (int t0 = 0; t0 < B.nc; t0 += MATCH_TC) {  // (uniform)
    const int nct = min(MATCH_TC, B.nc - t0);
    __syncthreads();  // the tile before has been read
    for (int i = tid; i < MATCH_TC * per_row; i += 256) {
      const int row = i / per_row, k0 = 16 * (i % per_row);
      match_v4 v = match_v4{0, 0, 0, 0};
      if (row < nct && k0 < dim) v = match_load16(desc + (size_t)(B.c0 + t0 + row) * dim + k0);
      *reinterpret_cast<match_v4 *>(s_cand + row * stride + k0) = v;
    }
    if (tid < MATCH_TC) {
      const int reg = (tid & 3) | ((tid >> 3) & 3) << 2;  // the accumulator register that holds row tid of its 32
      s_key[tid] = tid < nct ? 15 - reg - 16 * norm2[B.c0 + t0 + tid] : MATCH_PAD_KEY;
    }
    __syncthreads();
    if (!wave_on) continue;
#pragma unroll 1
    for (int sub = 0; sub < MATCH_TC / 32; ++sub) {
      if (sub * 32 >= nct) break;  // (uniform)
      match_v16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      const unsigned char *arow = s_cand + (sub * 32 + r) * stride + 16 * h;
#pragma unroll
      for (int s = 0; s < KS; ++s)
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(*reinterpret_cast<const match_v4 *>(arow + MATCH_KSTEP * s), qf[s], acc, 0, 0, 0);
      // the lane's 16 candidates of this tile: rows 8 g + 4 h + e, register 4 g + e
      int t1 = -MATCH_NONE - 1, t2 = -MATCH_NONE - 1;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const match_v4 kr = *reinterpret_cast<const match_v4 *>(s_key + sub * 32 + 8 * g + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int K = (acc[4 * g + e] << 5) + kr[e];
          if (SECOND) t2 = min(max(K, t2), t1);  // the median of the three, as t2 <= t1
          t1 = max(K, t1);
        }
      }
      const int v1 = -(t1 >> 4), reg = 15 - (t1 & 15), v2 = -(t2 >> 4);
      if (SECOND) b2 = min(max(b1, v1), min(b2, v2));  // the second of two ascending pairs
      i1 = v1 < b1 ? t0 + sub * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h : i1;
      b1 = min(v1, b1);
    }
  }
  if (!wave_on) return;
  // the two halves of the wave hold disjoint candidates of one query (a half that saw padded rows only holds v >= 2^26 and loses)
  const int ob1 = __shfl_xor(b1, 32, 64), oi1 = __shfl_xor(i1, 32, 64), ob2 = __shfl_xor(b2, 32, 64);
  const bool mine = b1 < ob1 || (b1 == ob1 && (unsigned)i1 < (unsigned)oi1);  // (-1, "none", loses as the largest unsigned)
  const int w1 = mine ? b1 : ob1, wi = mine ? i1 : oi1;
  const int w2 = min(mine ? ob1 : b1, mine ? b2 : ob2);  // the loser's best against the winner's second
  if (h == 0 && ql < B.nq) {
    const int qn = norm2[B.q0 + ql];
    best[B.out0 + ql] = wi;
    best2[B.out0 + ql] = wi < 0 ? -1 : w1 + qn;
    if (SECOND) second2[B.out0 + ql] = w2 >= MATCH_PAD_V ? -1 : w2 + qn;
  }
}

// the k steps the kernel is instantiated for: the smallest power of two with 32 KS >= dim
inline int match_ksteps(int dim) {
  int ks = 1;
  while (MATCH_KSTEP * ks < dim) ks *= 2;
  return ks;
}

inline size_t match_nn_lds(int ks) { return sizeof(int) * MATCH_TC + (size_t)MATCH_TC * (MATCH_KSTEP * ks + 16); }

// the pair of query t of a chunk: the last p < n_pairs with qoff[p] <= t (pairs without queries are stepped over)
__device__ __forceinline__ int match_pair_of(const int *__restrict__ qoff, int n_pairs, int t) {
  int lo = 0, hi = n_pairs;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (qoff[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

// One thread per query of the chunk: rules 1 to 4, the first that holds.  code[t]; key[t] = 1 for a match (for the scan);
// part[4 blockIdx.x + c]: the workgroup's queries rejected by rule c + 1.
__global__ __launch_bounds__(256) void k_match_decide(int n_q, int n_pairs, const int *__restrict__ qoff, const int *__restrict__ roff,
                                                      const int *__restrict__ n_cand, const int *__restrict__ best, const int *__restrict__ best2,
                                                      const int *__restrict__ second2, const int *__restrict__ rbest, int use_ratio, double r2,
                                                      int mutual, long long max_dist2, unsigned char *__restrict__ code,
                                                      trk_u64 *__restrict__ key, int *__restrict__ part) {
  __shared__ int s_part[4][4];
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  int c = -1;
  if (t < n_q) {
    const int p = match_pair_of(qoff, n_pairs, (int)t), a = (int)t - qoff[p], b = best[t];
    if (n_cand[p] == 0) c = MATCH_NO_CANDIDATE;
    else if (max_dist2 >= 0 && (long long)best2[t] > max_dist2) c = MATCH_FAR;
    else if (use_ratio && match_ambiguous(best2[t], second2[t], r2)) c = MATCH_AMBIGUOUS;
    else if (mutual && rbest[roff[p] + b] != a) c = MATCH_NOT_MUTUAL;
    else c = MATCH_KEPT;
    code[t] = (unsigned char)c;
    key[t] = c == MATCH_KEPT;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int cnt = __popcll(__ballot(c == k + 1));
    if (lane == 0) s_part[wave][k] = cnt;
  }
  __syncthreads();
  if (threadIdx.x < 4) part[4 * blockIdx.x + threadIdx.x] = s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
}

// the matches to their places: [a, b] local to their images, and the distance
__global__ __launch_bounds__(256) void k_match_emit(int n_q, int n_pairs, const int *__restrict__ qoff, const unsigned char *__restrict__ code,
                                                    const trk_u64 *__restrict__ scan, const int *__restrict__ best, const int *__restrict__ best2,
                                                    int2 *__restrict__ kp_pairs, int *__restrict__ dist2) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_q || code[t] != MATCH_KEPT) return;
  const int p = match_pair_of(qoff, n_pairs, (int)t);
  const trk_u64 o = scan[t];
  kp_pairs[o] = make_int2((int)t - qoff[p], best[t]);
  dist2[o] = best2[t];
}

// ptr[p], p <= n_pairs: the matches before pair p of the chunk
__global__ __launch_bounds__(256) void k_match_pair_ptr(int n_q, int n_pairs, const int *__restrict__ qoff, const trk_u64 *__restrict__ scan,
                                                        const trk_u64 *__restrict__ total, long long *__restrict__ ptr) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p > n_pairs) return;
  ptr[p] = (long long)(p < n_pairs && qoff[p] < n_q ? scan[qoff[p]] : *total);
}

template <int KS, bool SECOND>
int match_launch_ks(int n_blocks, const MatchBlock *blocks, const unsigned char *desc, int dim, const int *norm2, int *best, int *best2, int *second2) {
  const size_t lds = match_nn_lds(KS);
  MVBA_HIP(hipFuncSetAttribute((const void *)k_match_nn<KS, SECOND>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_match_nn<KS, SECOND>), dim3(n_blocks), dim3(256), lds, 0, blocks, desc, dim, norm2, best, best2, second2);
  MVBA_HIP(hipGetLastError());
  return MVBA_OK;
}

template <bool SECOND>
int match_launch_nn(int n_blocks, const MatchBlock *blocks, const unsigned char *desc, int dim, const int *norm2, int *best, int *best2, int *second2) {
  if (n_blocks == 0) return MVBA_OK;
  switch (match_ksteps(dim)) {
    case 1: return match_launch_ks<1, SECOND>(n_blocks, blocks, desc, dim, norm2, best, best2, second2);
    case 2: return match_launch_ks<2, SECOND>(n_blocks, blocks, desc, dim, norm2, best, best2, second2);
    case 4: return match_launch_ks<4, SECOND>(n_blocks, blocks, desc, dim, norm2, best, best2, second2);
    case 8: return match_launch_ks<8, SECOND>(n_blocks, blocks, desc, dim, norm2, best, best2, second2);
    default: return match_launch_ks<16, SECOND>(n_blocks, blocks, desc, dim, norm2, best, best2, second2);
  }
}

// the blocks of the directed job (query image q, candidate image c), its results from row `out` on
void match_add_blocks(std::vector<MatchBlock> &blocks, const int64_t *kp_ptr, int q, int c, int out) {
  const int q0 = (int)kp_ptr[q], nq = (int)(kp_ptr[q + 1] - kp_ptr[q]), c0 = (int)kp_ptr[c], nc = (int)(kp_ptr[c + 1] - kp_ptr[c]);
  for (int at = 0; at < nq; at += MATCH_TQ) blocks.push_back(MatchBlock{q0 + at, std::min(MATCH_TQ, nq - at), c0, nc, out + at});
}

}  // namespace

extern "C" {

int mvba_match_descriptors(int32_t n_images, const int64_t *kp_ptr, const uint8_t *desc, int32_t dim, const int32_t *pairs, int32_t n_pairs,
                           double ratio, int32_t mutual, int64_t max_dist2, int64_t *match_ptr, int32_t *kp_pairs, int32_t *dist2,
                           int32_t *nn_best, int32_t *nn_dist2, int32_t *nn_second2, int64_t *counts, double *timings_ms, int32_t device) {
  InitClock clk;
  int64_t Q = 0;
  int rc = match_check_args(n_images, kp_ptr, desc, dim, pairs, n_pairs, ratio, match_ptr, kp_pairs, dist2, counts, &Q);
  if (rc) return rc;
  for (int i = 0; i < MATCH_N_COUNTS; ++i) counts[i] = 0;
  if (timings_ms) timings_ms[0] = timings_ms[1] = timings_ms[2] = timings_ms[3] = 0.0;
  for (int32_t p = 0; p <= n_pairs; ++p) match_ptr[p] = 0;
  counts[MATCH_C_QUERIES] = Q;
  if (Q == 0) return MVBA_OK;
  if (device >= 0) MVBA_HIP(hipSetDevice(device));
  const int n = (int)kp_ptr[n_images];
  const bool use_ratio = ratio > 0.0, both = mutual != 0;
  const double r2 = match_ratio2(ratio);

  // ---- the chunks, and the largest of each buffer any of them needs
  std::vector<int32_t> cut{0};
  size_t max_q = 0, max_r = 0, max_p = 0;
  while (cut.back() < n_pairs) {
    const int32_t p0 = cut.back(), p1 = match_chunk_end(kp_ptr, pairs, n_pairs, p0, both, MATCH_CHUNK_QUERIES);
    size_t q = 0, r = 0;
    for (int32_t p = p0; p < p1; ++p) {
      q += (size_t)(kp_ptr[pairs[2 * p] + 1] - kp_ptr[pairs[2 * p]]);
      r += (size_t)(kp_ptr[pairs[2 * p + 1] + 1] - kp_ptr[pairs[2 * p + 1]]);
    }
    max_q = std::max(max_q, q);
    max_r = std::max(max_r, both ? r : 0);
    max_p = std::max(max_p, (size_t)(p1 - p0));
    cut.push_back(p1);
  }
  const size_t max_blocks = (max_q + max_r) / MATCH_TQ + 2 * max_p + 1, max_dec = (max_q + 255) / 256, max_sb = (max_q + TRK_SCAN_BLOCK - 1) / TRK_SCAN_BLOCK;

  DevBufs tmp;
  unsigned char *ddesc = nullptr, *dcode = nullptr;
  int *dnorm = nullptr, *dbest = nullptr, *dd1 = nullptr, *dd2 = nullptr, *drbest = nullptr, *drd1 = nullptr, *dqoff = nullptr, *droff = nullptr;
  int *dncand = nullptr, *dpart = nullptr, *ddist = nullptr;
  int2 *dkp = nullptr;
  MatchBlock *dblocks = nullptr;
  trk_u64 *dkey = nullptr, *dscan = nullptr, *dsums = nullptr, *dtotal = nullptr;
  long long *dptr = nullptr;
  if ((rc = tmp.alloc(&ddesc, (size_t)n * dim)) || (rc = tmp.alloc(&dnorm, (size_t)n)) || (rc = tmp.alloc(&dbest, max_q)) ||
      (rc = tmp.alloc(&dd1, max_q)) || (rc = tmp.alloc(&dd2, max_q)) || (rc = tmp.alloc(&drbest, max_r)) || (rc = tmp.alloc(&drd1, max_r)) ||
      (rc = tmp.alloc(&dqoff, max_p + 1)) || (rc = tmp.alloc(&droff, max_p + 1)) || (rc = tmp.alloc(&dncand, max_p)) ||
      (rc = tmp.alloc(&dpart, 4 * max_dec)) || (rc = tmp.alloc(&ddist, max_q)) || (rc = tmp.alloc(&dkp, max_q)) ||
      (rc = tmp.alloc(&dblocks, max_blocks)) || (rc = tmp.alloc(&dcode, max_q)) || (rc = tmp.alloc(&dkey, max_q)) ||
      (rc = tmp.alloc(&dscan, max_q)) || (rc = tmp.alloc(&dsums, max_sb)) || (rc = tmp.alloc(&dtotal, 1)) || (rc = tmp.alloc(&dptr, max_p + 1)))
    return rc;
  MVBA_HIP(hipMemcpy(ddesc, desc, (size_t)n * dim, hipMemcpyHostToDevice));
  if (timings_ms) timings_ms[0] = clk.lap();
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  EvGuard guard{ev, 3};
  for (auto &e : ev) MVBA_HIP(hipEventCreate(&e));
  double t_dist = 0.0, t_test = 0.0;

  hipEventRecord(ev[0], 0);
  hipLaunchKernelGGL(k_match_norm, dim3(trk_grid(n)), dim3(256), 0, 0, n, (int)dim, ddesc, dnorm);
  MVBA_HIP(hipGetLastError());

  std::vector<MatchBlock> fwd, rev;
  std::vector<int> qoff, roff, ncand, part;
  std::vector<long long> ptr;
  int64_t m_base = 0, q_base = 0;
  static_assert(sizeof(int2) == 2 * sizeof(int32_t) && sizeof(long long) == sizeof(int64_t), "kp_pairs and match_ptr travel as they are");
  for (size_t ch = 0; ch + 1 < cut.size(); ++ch) {
    const int32_t p0 = cut[ch], p1 = cut[ch + 1], P = p1 - p0;
    fwd.clear(); rev.clear();
    qoff.assign((size_t)P + 1, 0); roff.assign((size_t)P + 1, 0); ncand.assign((size_t)P, 0);
    for (int32_t i = 0; i < P; ++i) {
      const int k = pairs[2 * (p0 + i)], l = pairs[2 * (p0 + i) + 1];
      const int nk = (int)(kp_ptr[k + 1] - kp_ptr[k]), nl = (int)(kp_ptr[l + 1] - kp_ptr[l]);
      match_add_blocks(fwd, kp_ptr, k, l, qoff[i]);
      if (both) match_add_blocks(rev, kp_ptr, l, k, roff[i]);
      qoff[i + 1] = qoff[i] + nk;
      roff[i + 1] = roff[i] + (both ? nl : 0);
      ncand[i] = nl;
    }
    const int Qc = qoff[P];
    if (Qc == 0) {  // (pairs without queries: nothing to ask)
      for (int32_t i = 0; i <= P; ++i) match_ptr[p0 + i] = m_base;
      continue;
    }
    if (ch > 0) hipEventRecord(ev[0], 0);  // (the first chunk's lap holds the norms)
    // ---- distances: the nearest two forwards, the nearest backwards
    const size_t nf = fwd.size(), nr = rev.size();
    if (nf + nr > max_blocks) return fail(MVBA_ERR_STATE, "mvba_match_descriptors: " + std::to_string(nf + nr) + " blocks for " + std::to_string(max_blocks));
    MVBA_HIP(hipMemcpy(dblocks, fwd.data(), sizeof(MatchBlock) * nf, hipMemcpyHostToDevice));
    if (nr) MVBA_HIP(hipMemcpy(dblocks + nf, rev.data(), sizeof(MatchBlock) * nr, hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(dqoff, qoff.data(), sizeof(int) * ((size_t)P + 1), hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(droff, roff.data(), sizeof(int) * ((size_t)P + 1), hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(dncand, ncand.data(), sizeof(int) * (size_t)P, hipMemcpyHostToDevice));
    if ((rc = match_launch_nn<true>((int)nf, dblocks, ddesc, dim, dnorm, dbest, dd1, dd2))) return rc;
    if ((rc = match_launch_nn<false>((int)nr, dblocks + nf, ddesc, dim, dnorm, drbest, drd1, nullptr))) return rc;
    hipEventRecord(ev[1], 0);
    // ---- the tests, the scan, the matches to their places
    const unsigned gq = trk_grid(Qc);
    hipLaunchKernelGGL(k_match_decide, dim3(gq), dim3(256), 0, 0, Qc, (int)P, dqoff, droff, dncand, dbest, dd1, dd2, drbest, (int)use_ratio, r2,
                       (int)both, (long long)max_dist2, dcode, dkey, dpart);
    tracks_scan(Qc, dkey, dscan, dsums, dtotal);
    hipLaunchKernelGGL(k_match_emit, dim3(gq), dim3(256), 0, 0, Qc, (int)P, dqoff, dcode, dscan, dbest, dd1, dkp, ddist);
    hipLaunchKernelGGL(k_match_pair_ptr, dim3(trk_grid((long long)P + 1)), dim3(256), 0, 0, Qc, (int)P, dqoff, dscan, dtotal, dptr);
    hipEventRecord(ev[2], 0);
    MVBA_HIP(hipGetLastError());
    // ---- this chunk's part of the answer
    ptr.resize((size_t)P + 1);
    MVBA_HIP(hipMemcpy(ptr.data(), dptr, sizeof(long long) * ((size_t)P + 1), hipMemcpyDeviceToHost));
    for (int32_t i = 0; i <= P; ++i) match_ptr[p0 + i] = m_base + ptr[i];
    const int64_t got = ptr[P];
    if (got) {
      MVBA_HIP(hipMemcpy(kp_pairs + 2 * m_base, dkp, sizeof(int2) * (size_t)got, hipMemcpyDeviceToHost));
      MVBA_HIP(hipMemcpy(dist2 + m_base, ddist, sizeof(int) * (size_t)got, hipMemcpyDeviceToHost));
    }
    if (nn_best) MVBA_HIP(hipMemcpy(nn_best + q_base, dbest, sizeof(int) * (size_t)Qc, hipMemcpyDeviceToHost));
    if (nn_dist2) MVBA_HIP(hipMemcpy(nn_dist2 + q_base, dd1, sizeof(int) * (size_t)Qc, hipMemcpyDeviceToHost));
    if (nn_second2) MVBA_HIP(hipMemcpy(nn_second2 + q_base, dd2, sizeof(int) * (size_t)Qc, hipMemcpyDeviceToHost));
    part.resize(4 * (size_t)gq);
    MVBA_HIP(hipMemcpy(part.data(), dpart, sizeof(int) * part.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < part.size(); ++i) counts[MATCH_C_NO_CANDIDATE + (i & 3)] += part[i];
    m_base += got;
    q_base += Qc;
    float f1 = 0.f, f2 = 0.f;
    hipEventElapsedTime(&f1, ev[0], ev[1]);
    hipEventElapsedTime(&f2, ev[1], ev[2]);
    t_dist += f1;
    t_test += f2;
  }
  counts[MATCH_C_MATCHES] = m_base;
  if (timings_ms) {
    timings_ms[1] = t_dist;
    timings_ms[2] = t_test;
    timings_ms[3] = std::max(0.0, clk.lap() - t_dist - t_test);
  }
  return MVBA_OK;
}

}  // extern "C"
