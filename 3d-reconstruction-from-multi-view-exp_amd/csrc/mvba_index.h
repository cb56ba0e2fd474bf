// The Schur index of the gather forms, built on the device (mvba_create) -- kernels, gfx950: k_idx_count, k_idx_scan, k_idx_fill
// (stable counting sort of the items by camera pair), k_idx_bounds, k_idx_merge (sub-lists into step-major rows, wave by wave),
// k_idx_interleave (one LDS-DMA row per step).
//
// Included by mvba.hip inside its device-code namespace, after mvba_tail.h: needs nothing from the headers before it, only
// wave_sync of mvba_common.h.  The host side that sizes and launches these is mvba_create.h.

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
// (W = 21: 64 ints = 256 bytes with 1 int of padding; W = 64: two words per item, w0[64] | w1[64] = 512 bytes -- lane_idx_pack,
// mvba_engine_host.h; decide_schur_form has checked that every item packs)
__global__ void k_idx_interleave(long long n_steps, int W, int row, const int *__restrict__ st_k, const int *__restrict__ st_l,
                                 const int *__restrict__ st_a, int *__restrict__ out) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_steps * row) return;
  const long long st = t / row;
  const int e = (int)(t - st * row), which = e / W, sl = e - which * W;
  if (W == LANES_W) {
    const long long o = st * W + sl;
    const LaneIdx p = lane_idx_pack(st_k[o], st_l[o], st_a[o]);
    out[t] = (int)(which == 0 ? p.w0 : p.w1);
    return;
  }
  const int *src = which == 0 ? st_k : (which == 1 ? st_l : st_a);
  out[t] = which < 3 ? src[st * W + sl] : 0;
}
