// Matching of uint8 descriptors (mvba_match_descriptors) -- kernels and host code, gfx950.
//
// Included by mvba.hip after mvba_tracks.h: uses its tracks_scan and trk_u64, mvba_tracks_host.h's trk_grid, mvba_start.h's
// InitClock and EvLaps, mvba.hip's DevBufs, fail and MVBA_HIP, and mvba_match_host.h's MatchBlock, checks, plan (match_plan),
// chunk lists (match_chunk_lists) and ratio test.  Nothing here runs on the LM path.  
//
// The host side in stages: the plan and the lists are mvba_match_host.h's; MatchDev owns the device buffers, match_chunk_run
// uploads and launches one chunk, match_chunk_read brings its part of the answer back; the entry point strings them together.
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

// The device buffers of a call, each as large as the largest chunk of the plan needs it; freed when the owner goes.
struct MatchDev {
  DevBufs tmp;
  unsigned char *desc = nullptr, *code = nullptr;                                        // [n][dim]; the rule of a query
  int *norm = nullptr;                                                                   // [n]
  int *best = nullptr, *d1 = nullptr, *d2 = nullptr, *rbest = nullptr, *rd1 = nullptr;   // per query row, forwards and backwards
  int *qoff = nullptr, *roff = nullptr, *ncand = nullptr, *part = nullptr, *dist = nullptr;
  int2 *kp = nullptr;
  MatchBlock *blocks = nullptr;  // fwd, then rev
  trk_u64 *key = nullptr, *scan = nullptr, *sums = nullptr, *total = nullptr;
  long long *ptr = nullptr;
  size_t max_blocks = 0;
  int n = 0, dim = 0;

  int alloc(const MatchPlan &pl, int n_nodes, int dim_) {
    int rc;
    n = n_nodes, dim = dim_, max_blocks = pl.max_blocks;
    if ((rc = tmp.alloc(&desc, (size_t)n * dim)) || (rc = tmp.alloc(&norm, (size_t)n)) || (rc = tmp.alloc(&best, pl.max_q)) ||
        (rc = tmp.alloc(&d1, pl.max_q)) || (rc = tmp.alloc(&d2, pl.max_q)) || (rc = tmp.alloc(&rbest, pl.max_r)) || (rc = tmp.alloc(&rd1, pl.max_r)) ||
        (rc = tmp.alloc(&qoff, pl.max_p + 1)) || (rc = tmp.alloc(&roff, pl.max_p + 1)) || (rc = tmp.alloc(&ncand, pl.max_p)) ||
        (rc = tmp.alloc(&part, 4 * pl.max_dec)) || (rc = tmp.alloc(&dist, pl.max_q)) || (rc = tmp.alloc(&kp, pl.max_q)) ||
        (rc = tmp.alloc(&blocks, pl.max_blocks)) || (rc = tmp.alloc(&code, pl.max_q)) || (rc = tmp.alloc(&key, pl.max_q)) ||
        (rc = tmp.alloc(&scan, pl.max_q)) || (rc = tmp.alloc(&sums, pl.max_sb)) || (rc = tmp.alloc(&total, 1)) || (rc = tmp.alloc(&ptr, pl.max_p + 1)))
      return rc;
    return MVBA_OK;
  }
};

// rules 2 to 4 as the caller set them
struct MatchRules {
  bool use_ratio, mutual;
  double r2;
  long long max_dist2;
};

// One chunk on the device: its lists up, the distances (mark 1 after them), then the tests, the scan and the matches to their
// places (mark 2).  restart: mark 0 is recorded again first -- not in the first chunk, whose lap holds the norms.
int match_chunk_run(MatchDev &d, const MatchLists &L, const MatchRules &rules, bool restart, EvLaps &ev) {
  int rc;
  if (restart) ev.again(0);
  const size_t nf = L.fwd.size(), nr = L.rev.size(), P = (size_t)L.P;
  if (nf + nr > d.max_blocks) return fail(MVBA_ERR_STATE, "mvba_match_descriptors: " + std::to_string(nf + nr) + " blocks for " + std::to_string(d.max_blocks));
  MVBA_HIP(hipMemcpy(d.blocks, L.fwd.data(), sizeof(MatchBlock) * nf, hipMemcpyHostToDevice));
  if (nr) MVBA_HIP(hipMemcpy(d.blocks + nf, L.rev.data(), sizeof(MatchBlock) * nr, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(d.qoff, L.qoff.data(), sizeof(int) * (P + 1), hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(d.roff, L.roff.data(), sizeof(int) * (P + 1), hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(d.ncand, L.ncand.data(), sizeof(int) * P, hipMemcpyHostToDevice));
  if ((rc = match_launch_nn<true>((int)nf, d.blocks, d.desc, d.dim, d.norm, d.best, d.d1, d.d2))) return rc;
  if ((rc = match_launch_nn<false>((int)nr, d.blocks + nf, d.desc, d.dim, d.norm, d.rbest, d.rd1, nullptr))) return rc;
  ev.mark();
  const unsigned gq = trk_grid(L.Qc);
  hipLaunchKernelGGL(k_match_decide, dim3(gq), dim3(256), 0, 0, L.Qc, L.P, d.qoff, d.roff, d.ncand, d.best, d.d1, d.d2, d.rbest, (int)rules.use_ratio,
                     rules.r2, (int)rules.mutual, rules.max_dist2, d.code, d.key, d.part);
  tracks_scan(L.Qc, d.key, d.scan, d.sums, d.total);
  hipLaunchKernelGGL(k_match_emit, dim3(gq), dim3(256), 0, 0, L.Qc, L.P, d.qoff, d.code, d.scan, d.best, d.d1, d.kp, d.dist);
  hipLaunchKernelGGL(k_match_pair_ptr, dim3(trk_grid((long long)P + 1)), dim3(256), 0, 0, L.Qc, L.P, d.qoff, d.scan, d.total, d.ptr);
  ev.mark();
  MVBA_HIP(hipGetLastError());
  return MVBA_OK;
}

// the caller's arrays, and how far the chunks so far have filled them: m_base matches, q_base queries
struct MatchOut {
  int64_t *match_ptr;
  int32_t *kp_pairs, *dist2, *nn_best, *nn_dist2, *nn_second2;
  int64_t *counts;
  int64_t m_base = 0, q_base = 0;
};

// A chunk's part of the answer: match_ptr of its pairs (from p0 on) rebased by the matches before it, its matches, the
// per-query arrays that were asked for, and the workgroups' partial counts added up.
int match_chunk_read(const MatchDev &d, const MatchLists &L, int32_t p0, MatchOut &out) {
  static_assert(sizeof(int2) == 2 * sizeof(int32_t) && sizeof(long long) == sizeof(int64_t), "kp_pairs and match_ptr travel as they are");
  const size_t P = (size_t)L.P, Qc = (size_t)L.Qc;
  std::vector<long long> ptr(P + 1);
  MVBA_HIP(hipMemcpy(ptr.data(), d.ptr, sizeof(long long) * (P + 1), hipMemcpyDeviceToHost));
  for (size_t i = 0; i <= P; ++i) out.match_ptr[p0 + i] = out.m_base + ptr[i];
  const int64_t got = ptr[P];
  if (got) {
    MVBA_HIP(hipMemcpy(out.kp_pairs + 2 * out.m_base, d.kp, sizeof(int2) * (size_t)got, hipMemcpyDeviceToHost));
    MVBA_HIP(hipMemcpy(out.dist2 + out.m_base, d.dist, sizeof(int) * (size_t)got, hipMemcpyDeviceToHost));
  }
  if (out.nn_best) MVBA_HIP(hipMemcpy(out.nn_best + out.q_base, d.best, sizeof(int) * Qc, hipMemcpyDeviceToHost));
  if (out.nn_dist2) MVBA_HIP(hipMemcpy(out.nn_dist2 + out.q_base, d.d1, sizeof(int) * Qc, hipMemcpyDeviceToHost));
  if (out.nn_second2) MVBA_HIP(hipMemcpy(out.nn_second2 + out.q_base, d.d2, sizeof(int) * Qc, hipMemcpyDeviceToHost));
  std::vector<int> part(4 * (size_t)trk_grid(L.Qc));
  MVBA_HIP(hipMemcpy(part.data(), d.part, sizeof(int) * part.size(), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < part.size(); ++i) out.counts[MATCH_C_NO_CANDIDATE + (i & 3)] += part[i];
  out.m_base += got;
  out.q_base += L.Qc;
  return MVBA_OK;
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
  const MatchRules rules{ratio > 0.0, mutual != 0, match_ratio2(ratio), (long long)max_dist2};
  const MatchPlan plan = match_plan(kp_ptr, pairs, n_pairs, rules.mutual, MATCH_CHUNK_QUERIES);
  MatchDev d;
  if ((rc = d.alloc(plan, n, dim))) return rc;
  MVBA_HIP(hipMemcpy(d.desc, desc, (size_t)n * dim, hipMemcpyHostToDevice));
  if (timings_ms) timings_ms[0] = clk.lap();
  EvLaps ev;
  if ((rc = ev.create(3))) return rc;
  double t_dist = 0.0, t_test = 0.0;

  ev.mark();
  hipLaunchKernelGGL(k_match_norm, dim3(trk_grid(n)), dim3(256), 0, 0, n, (int)dim, d.desc, d.norm);
  MVBA_HIP(hipGetLastError());

  MatchLists L;
  MatchOut out{match_ptr, kp_pairs, dist2, nn_best, nn_dist2, nn_second2, counts};
  for (size_t ch = 0; ch + 1 < plan.cut.size(); ++ch) {
    const int32_t p0 = plan.cut[ch], p1 = plan.cut[ch + 1];
    match_chunk_lists(kp_ptr, pairs, p0, p1, rules.mutual, L);
    if (L.Qc == 0) {  // (pairs without queries: nothing to ask)
      for (int32_t p = p0; p <= p1; ++p) match_ptr[p] = out.m_base;
      continue;
    }
    if ((rc = match_chunk_run(d, L, rules, ch > 0, ev)) || (rc = match_chunk_read(d, L, p0, out))) return rc;
    t_dist += ev.ms(0, 1);
    t_test += ev.ms(1, 2);
  }
  counts[MATCH_C_MATCHES] = out.m_base;
  if (timings_ms) {
    timings_ms[1] = t_dist;
    timings_ms[2] = t_test;
    timings_ms[3] = lap_rest(clk.lap(), t_dist + t_test);
  }
  return MVBA_OK;
}

}  // extern "C"
