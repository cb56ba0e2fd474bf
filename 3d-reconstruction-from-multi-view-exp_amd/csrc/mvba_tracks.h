// Feature tracks from pairwise matches (mvba_build_tracks) -- kernels and host code, gfx950.
//
// Included by mvba.hip after mvba_start.h: uses its InitClock and EvLaps, mvba.hip's DevBufs, fail and MVBA_HIP, and
// mvba_tracks_host.h's checks, tracks_classify, trk_grid and TRK_SCAN_BLOCK.  mvba_match.h uses tracks_scan and trk_u64 of
// this header.  Nothing here runs on the LM path.  
//
// The host side in stages over one TracksDev, which owns the device buffers: tracks_upload, tracks_labels, tracks_candidates,
// tracks_survivors, tracks_download; the entry point is the checks, the five calls and the laps.
//
// Keypoint j of image i is node kp_ptr[i] + j; a match is an edge between two nodes; a track is a connected component of that
// graph with at most one node per image.  Integers only, and integer atomics only (atomicMin, atomicAdd, atomicOr): every
// output is a function of the edge SET, whatever the order of the edges or of the threads.
//
// Labels.  parent[v] <= v ALWAYS: it starts as v and is only ever lowered, to a node of v's own component.  So every walk
// v -> parent[v] -> ... strictly descends and ends after a number of steps the data alone bounds; no kernel waits for another
// thread or retries on its write.  A round is two launches: k_tracks_hook (one thread per edge: the roots of both ends, the
// larger root hooked under the smaller by atomicMin) and k_tracks_flatten (parent[v] <- root(v)).  A read of parent that
// misses another thread's write of the same launch returns an OLDER value -- still an ancestor in the same component, still
// <= v: the hook it leads to is a valid one, and whatever link an atomicMin replaces is put back by its edge in the next round.
// The host repeats rounds until one changes nothing; then every edge joins two nodes of one root, and a root is the smallest
// node of its component.  A round that changes something turns at least one root into a non-root for good: at most n_nodes
// rounds, in practice a handful.  Visibility from one launch to the next comes from the kernel boundary alone.
//
// Layout.  size[root] by atomicAdd; a component is classified by tracks_classify; the candidates get segments by an exclusive
// scan in ascending root order (count and size in the two halves of one 64-bit sum), are filled through an integer cursor per
// component and sorted by node id into a second buffer by counting ranks -- ids are distinct, so the sorted segment does not
// depend on the fill order: one lane per track up to 32 entries, one wave per longer track.  Node ids are image-major: two
// nodes of one image are neighbours in the sorted segment (k_tracks_conflict).  A second scan over the survivors numbers the
// tracks in ascending order of their smallest node and places their observations.

namespace {

typedef unsigned long long trk_u64;

constexpr int TRK_LANE_MAX = 32;            // entries up to which one lane ranks a whole track
constexpr int TRK_HOOK_GRID = 8192;         // workgroups of the hook kernel at most (a grid stride beyond)

// the root of v's tree: strictly descending, since parent[x] <= x whatever this thread gets to see of other threads' writes
__device__ __forceinline__ int trk_root(const int *parent, int v) {
  int p = parent[v];
  while (p < v) {
    v = p;
    p = parent[v];
  }
  return v;
}

// the image of node v: the last i < n_images with kp[i] <= v (images without keypoints are stepped over)
__device__ __forceinline__ int trk_image(const int *__restrict__ kp, int n_images, int v) {
  int lo = 0, hi = n_images;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (kp[mid] <= v) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_tracks_init(int n, int *__restrict__ parent) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v < n) parent[v] = (int)v;
}

// One thread per edge (a grid stride beyond TRK_HOOK_GRID workgroups).  *changed: set when an atomicMin lowered a parent.
__global__ __launch_bounds__(256) void k_tracks_hook(long long n_edges, const int2 *__restrict__ edges, const unsigned char *__restrict__ edge_ok,
                                                     int *parent, unsigned *changed) {
  const long long stride = (long long)gridDim.x * 256;
  bool any = false;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n_edges; e += stride) {
    if (edge_ok && !edge_ok[e]) continue;
    const int2 uv = edges[e];
    if (uv.x == uv.y) continue;
    const int ru = trk_root(parent, uv.x), rv = trk_root(parent, uv.y);
    if (ru == rv) continue;
    const int lo = min(ru, rv), hi = max(ru, rv);
    if (atomicMin(&parent[hi], lo) > lo) any = true;
  }
  if (__any(any) && (threadIdx.x & 63) == 0) atomicOr(changed, 1u);
}

__global__ __launch_bounds__(256) void k_tracks_flatten(int n, int *parent) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int r = trk_root(parent, (int)v);
  if (r < parent[v]) parent[v] = r;
}

__global__ __launch_bounds__(256) void k_tracks_sizes(int n, const int *__restrict__ label, int *__restrict__ size) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v < n) atomicAdd(&size[label[v]], 1);
}

// key[v] = (1 << 32 | size) at the root of a candidate (bad == nullptr) or of a surviving track (bad: the conflict marks), else 0
__global__ __launch_bounds__(256) void k_tracks_keys(int n, const int *__restrict__ label, const int *__restrict__ size,
                                                     const unsigned char *__restrict__ bad, int min_length, int n_images,
                                                     trk_u64 *__restrict__ key) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  trk_u64 k = 0;
  if (label[v] == (int)v) {
    const int s = size[v];
    if (tracks_classify(s, min_length, n_images) == TRK_CANDIDATE && !(bad && bad[v])) k = (1ull << 32) | (unsigned)s;
  }
  key[v] = k;
}

// the inclusive sum of x over the workgroup's 256 threads up to and including this one; total: over all of them
__device__ __forceinline__ trk_u64 trk_block_scan(trk_u64 x, trk_u64 (&s_w)[4], trk_u64 &total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const trk_u64 y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) s_w[w] = x;
  __syncthreads();
  trk_u64 before = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < w) before += s_w[i];
    total += s_w[i];
  }
  __syncthreads();  // (s_w is free for the next call)
  return before + x;
}

// Exclusive scan of key [n] in three launches: inside blocks of TRK_SCAN_BLOCK items (out, and the block's total into sums),
// over the totals (one workgroup; *total = everything), and the block's offset added.
__global__ __launch_bounds__(256) void k_tracks_scan_blocks(int n, const trk_u64 *__restrict__ key, trk_u64 *__restrict__ out,
                                                            trk_u64 *__restrict__ sums) {
  __shared__ trk_u64 s_w[4];
  const long long base = (long long)blockIdx.x * TRK_SCAN_BLOCK + (long long)threadIdx.x * TRK_SCAN_ITEMS;
  trk_u64 x[TRK_SCAN_ITEMS], mine = 0;
#pragma unroll
  for (int i = 0; i < TRK_SCAN_ITEMS; ++i) {
    x[i] = base + i < n ? key[base + i] : 0;
    mine += x[i];
  }
  trk_u64 total;
  trk_u64 run = trk_block_scan(mine, s_w, total) - mine;
#pragma unroll
  for (int i = 0; i < TRK_SCAN_ITEMS; ++i) {
    if (base + i < n) out[base + i] = run;
    run += x[i];
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_tracks_scan_sums(int nb, trk_u64 *__restrict__ sums, trk_u64 *__restrict__ total) {
  __shared__ trk_u64 s_w[4];
  trk_u64 carry = 0;
  for (int base = 0; base < nb; base += 256) {  // (uniform)
    const int i = base + threadIdx.x;
    const trk_u64 x = i < nb ? sums[i] : 0;
    trk_u64 all;
    const trk_u64 incl = trk_block_scan(x, s_w, all);
    if (i < nb) sums[i] = carry + incl - x;
    carry += all;
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void k_tracks_scan_add(int n, trk_u64 *__restrict__ out, const trk_u64 *__restrict__ sums) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v < n) out[v] += sums[v / TRK_SCAN_BLOCK];
}

// the candidates in ascending root order: cand_root[c]
__global__ __launch_bounds__(256) void k_tracks_cands(int n, const trk_u64 *__restrict__ key, const trk_u64 *__restrict__ scan,
                                                      int *__restrict__ cand_root) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v < n && key[v]) cand_root[scan[v] >> 32] = (int)v;
}

// every node of a candidate into its component's segment, at the place its cursor hands out (below size[root]: one per node)
__global__ __launch_bounds__(256) void k_tracks_fill(int n, const int *__restrict__ label, const trk_u64 *__restrict__ key,
                                                     const trk_u64 *__restrict__ scan, int *__restrict__ cursor, int *__restrict__ seg) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int r = label[v];
  if (!key[r]) return;
  seg[(unsigned)scan[r] + (unsigned)atomicAdd(&cursor[r], 1)] = (int)v;
}

// entries i0, i0 + step, ... of the segment seg[s .. s + len) to their ranks in sorted[s ..), with their images beside them
__device__ __forceinline__ void trk_rank(const int *__restrict__ seg, unsigned s, int len, int i0, int step, const int *__restrict__ kp,
                                         int n_images, int *__restrict__ sorted, int *__restrict__ cam_sorted) {
  for (int i = i0; i < len; i += step) {
    const int v = seg[s + i];
    int rank = 0;
    for (int j = 0; j < len; ++j) rank += seg[s + j] < v;
    sorted[s + rank] = v;
    cam_sorted[s + rank] = trk_image(kp, n_images, v);
  }
}

// Thread c: candidate c.  Up to TRK_LANE_MAX entries the lane ranks its own track; the longer tracks of a wave's 64 candidates
// are then taken one after the other by the whole wave.
__global__ __launch_bounds__(256) void k_tracks_sort(int n_cand, const int *__restrict__ cand_root, const trk_u64 *__restrict__ scan,
                                                     const int *__restrict__ size, const int *__restrict__ seg, const int *__restrict__ kp,
                                                     int n_images, int *__restrict__ sorted, int *__restrict__ cam_sorted) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int len = 0;
  unsigned s = 0;
  if (c < n_cand) {
    const int r = cand_root[c];
    len = size[r];
    s = (unsigned)scan[r];
  }
  if (len <= TRK_LANE_MAX) trk_rank(seg, s, len, 0, 1, kp, n_images, sorted, cam_sorted);
  trk_u64 longer = __ballot(len > TRK_LANE_MAX);
  while (longer) {  // (uniform)
    const int q = __ffsll((long long)longer) - 1;
    longer &= longer - 1;
    trk_rank(seg, (unsigned)__shfl((int)s, q, 64), __shfl(len, q, 64), lane, 64, kp, n_images, sorted, cam_sorted);
  }
}

// two neighbours of a sorted segment in one image: the component is marked (every writer writes the same 1)
__global__ __launch_bounds__(256) void k_tracks_conflict(int n_ent, const int *__restrict__ sorted, const int *__restrict__ cam_sorted,
                                                         const int *__restrict__ label, unsigned char *__restrict__ bad) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p < 1 || p >= n_ent || cam_sorted[p] != cam_sorted[p - 1]) return;
  const int r = label[sorted[p]];
  if (label[sorted[p - 1]] == r) bad[r] = 1;
}

// the observations of the surviving tracks: entry p of the sorted buffer to its place in the output
__global__ __launch_bounds__(256) void k_tracks_out_obs(int n_ent, const int *__restrict__ sorted, const int *__restrict__ cam_sorted,
                                                        const int *__restrict__ label, const unsigned char *__restrict__ bad,
                                                        const trk_u64 *__restrict__ scan1, const trk_u64 *__restrict__ scan2,
                                                        const double2 *__restrict__ kp_xy, int *__restrict__ obs_node,
                                                        int *__restrict__ cam_idx, double2 *__restrict__ xy) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_ent) return;
  const int v = sorted[p], r = label[v];
  if (bad[r]) return;
  const unsigned o = (unsigned)scan2[r] + ((unsigned)p - (unsigned)scan1[r]);
  obs_node[o] = v;
  cam_idx[o] = cam_sorted[p];
  if (xy) xy[o] = kp_xy[v];
}

// node_track of every node; at a root the component's counts, and the start of a surviving track.  cnt [TRK_N_COUNTS].
__global__ __launch_bounds__(256) void k_tracks_out_nodes(int n, const int *__restrict__ label, const int *__restrict__ size,
                                                          const unsigned char *__restrict__ bad, const trk_u64 *__restrict__ scan2,
                                                          int min_length, int n_images, int *__restrict__ node_track,
                                                          long long *__restrict__ pt_ptr, trk_u64 *__restrict__ cnt) {
  __shared__ trk_u64 s_c[TRK_N_COUNTS];
  if (threadIdx.x < TRK_N_COUNTS) s_c[threadIdx.x] = 0;
  __syncthreads();
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v < n) {
    const int r = label[v], s = size[r], cls = tracks_classify(s, min_length, n_images);
    const bool root = r == (int)v, conflict = cls == TRK_CANDIDATE && bad[r];
    int code = TRK_UNMATCHED;
    if (cls == TRK_SHORT) code = TRK_TOO_SHORT;
    else if (cls == TRK_OVERSIZE || conflict) code = TRK_DROPPED;
    else if (cls == TRK_CANDIDATE) code = (int)(scan2[r] >> 32);
    node_track[v] = code;
    if (root) {
      if (cls == TRK_SINGLETON) atomicAdd(&s_c[TRK_C_SINGLETONS], 1ull);
      else atomicAdd(&s_c[TRK_C_COMPONENTS], 1ull);
      if (cls == TRK_SHORT) atomicAdd(&s_c[TRK_C_SHORT], 1ull);
      if (cls == TRK_OVERSIZE) {
        atomicAdd(&s_c[TRK_C_OVERSIZE], 1ull);
        atomicAdd(&s_c[TRK_C_OVERSIZE_NODES], (trk_u64)s);
      }
      if (conflict) {
        atomicAdd(&s_c[TRK_C_CONFLICT], 1ull);
        atomicAdd(&s_c[TRK_C_CONFLICT_NODES], (trk_u64)s);
      }
      if (code >= 0) pt_ptr[code] = (long long)(unsigned)scan2[r];
    }
  }
  __syncthreads();
  if (threadIdx.x < TRK_N_COUNTS && s_c[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], s_c[threadIdx.x]);
}

// the three launches of an exclusive scan of key [n] into out [n]; *total (device) = the sum of all of it
void tracks_scan(int n, const trk_u64 *key, trk_u64 *out, trk_u64 *sums, trk_u64 *total) {
  const int nb = (int)(((long long)n + TRK_SCAN_BLOCK - 1) / TRK_SCAN_BLOCK);
  hipLaunchKernelGGL(k_tracks_scan_blocks, dim3(nb), dim3(256), 0, 0, n, key, out, sums);
  hipLaunchKernelGGL(k_tracks_scan_sums, dim3(1), dim3(256), 0, 0, nb, sums, total);
  hipLaunchKernelGGL(k_tracks_scan_add, dim3(trk_grid(n)), dim3(256), 0, 0, n, out, sums);
}

// The device buffers of a call and the sizes the stages hand on; freed when the owner goes.
struct TracksDev {
  DevBufs tmp;
  int n = 0, n_images = 0, min_length = 0;  // nodes, images, the shortest track
  long long n_edges = 0;
  int n_cand = 0, n_ent = 0, n_tracks = 0, n_obs = 0;  // candidates and their nodes (tracks_candidates); survivors and theirs (tracks_survivors)
  // tracks_upload; edge and ok [n_edges] are released once the labels stand
  int2 *edge = nullptr;
  unsigned char *ok = nullptr;
  int *kp = nullptr, *parent = nullptr;  // [n_images + 1]; [n]: the labels once they have settled
  unsigned *changed = nullptr;
  double2 *kpxy = nullptr;
  // tracks_candidates: [n] each, then cand [n_cand] and seg, sorted, cam [n_ent]
  int *size = nullptr, *cursor = nullptr, *track = nullptr, *cand = nullptr, *sorted = nullptr, *cam = nullptr;
  int *seg = nullptr;  // the unsorted segments; once k_tracks_sort has read them, the cam_idx of the output (n_obs <= n_ent)
  unsigned char *bad = nullptr;
  trk_u64 *key = nullptr, *scan1 = nullptr, *scan2 = nullptr, *sums = nullptr, *total = nullptr, *cnt = nullptr;
  // tracks_survivors: ptr [n_tracks + 1], obs and xy [n_obs]
  long long *ptr = nullptr;
  int *obs = nullptr;
  double2 *xy = nullptr;
};

// the offsets (as int), the edges, their flags and the positions to the device
int tracks_upload(TracksDev &d, const int64_t *kp_ptr, const double *kp_xy, const int32_t *edges, const uint8_t *edge_ok, bool want_xy) {
  static_assert(sizeof(int2) == 2 * sizeof(int32_t), "edges travel as they are");
  int rc;
  const size_t ne = (size_t)d.n_edges;
  if ((rc = d.tmp.alloc(&d.edge, ne)) || (rc = d.tmp.alloc(&d.kp, (size_t)d.n_images + 1)) || (rc = d.tmp.alloc(&d.parent, (size_t)d.n)) ||
      (rc = d.tmp.alloc(&d.changed, 1)))
    return rc;
  if (edge_ok && (rc = d.tmp.alloc(&d.ok, ne))) return rc;
  if (want_xy && (rc = d.tmp.alloc(&d.kpxy, (size_t)d.n))) return rc;
  std::vector<int> kp32((size_t)d.n_images + 1);
  for (int32_t i = 0; i <= d.n_images; ++i) kp32[i] = (int)kp_ptr[i];
  MVBA_HIP(hipMemcpy(d.kp, kp32.data(), sizeof(int) * kp32.size(), hipMemcpyHostToDevice));
  if (ne) MVBA_HIP(hipMemcpy(d.edge, edges, sizeof(int2) * ne, hipMemcpyHostToDevice));
  if (d.ok && ne) MVBA_HIP(hipMemcpy(d.ok, edge_ok, ne, hipMemcpyHostToDevice));
  if (d.kpxy) MVBA_HIP(hipMemcpy(d.kpxy, kp_xy, sizeof(double2) * (size_t)d.n, hipMemcpyHostToDevice));
  return MVBA_OK;
}

// hook and flatten until a round changes nothing: d.parent is then every node's label.  *rounds: how many it took.
int tracks_labels(TracksDev &d, int64_t *rounds) {
  const int n = d.n;
  hipLaunchKernelGGL(k_tracks_init, dim3(trk_grid(n)), dim3(256), 0, 0, n, d.parent);
  *rounds = 0;
  const unsigned hook_grid = (unsigned)std::min<long long>(TRK_HOOK_GRID, trk_grid(d.n_edges));
  for (unsigned changed = d.n_edges > 0; changed;) {
    if (*rounds > n)  // (every changing round costs a root: the loop cannot get here)
      return fail(MVBA_ERR_STATE, "mvba_build_tracks: the labels did not settle in n_nodes + 1 = " + std::to_string((int64_t)n + 1) + " rounds");
    MVBA_HIP(hipMemsetAsync(d.changed, 0, sizeof(unsigned), 0));
    hipLaunchKernelGGL(k_tracks_hook, dim3(hook_grid), dim3(256), 0, 0, d.n_edges, d.edge, d.ok, d.parent, d.changed);
    hipLaunchKernelGGL(k_tracks_flatten, dim3(trk_grid(n)), dim3(256), 0, 0, n, d.parent);
    MVBA_HIP(hipGetLastError());
    MVBA_HIP(hipMemcpy(&changed, d.changed, sizeof(unsigned), hipMemcpyDeviceToHost));
    ++*rounds;
  }
  return MVBA_OK;
}

// Sizes, the candidates and their segments, sorted, and the conflicts marked.  The edges and their flags go first -- the
// labels hold all they said -- so that they and the buffers of the layout are never there together.
int tracks_candidates(TracksDev &d) {
  int rc;
  const int n = d.n;
  const size_t nn = (size_t)n, nb = (nn + TRK_SCAN_BLOCK - 1) / TRK_SCAN_BLOCK;
  d.tmp.release(d.edge);
  d.tmp.release(d.ok);
  if ((rc = d.tmp.alloc(&d.size, nn)) || (rc = d.tmp.alloc(&d.cursor, nn)) || (rc = d.tmp.alloc(&d.bad, nn)) || (rc = d.tmp.alloc(&d.key, nn)) ||
      (rc = d.tmp.alloc(&d.scan1, nn)) || (rc = d.tmp.alloc(&d.scan2, nn)) || (rc = d.tmp.alloc(&d.sums, nb)) || (rc = d.tmp.alloc(&d.total, 2)) ||
      (rc = d.tmp.alloc(&d.cnt, TRK_N_COUNTS)) || (rc = d.tmp.alloc(&d.track, nn)))
    return rc;
  MVBA_HIP(hipMemsetAsync(d.size, 0, sizeof(int) * nn, 0));
  MVBA_HIP(hipMemsetAsync(d.cursor, 0, sizeof(int) * nn, 0));
  MVBA_HIP(hipMemsetAsync(d.bad, 0, nn, 0));
  MVBA_HIP(hipMemsetAsync(d.cnt, 0, sizeof(trk_u64) * TRK_N_COUNTS, 0));
  const int *label = d.parent;
  hipLaunchKernelGGL(k_tracks_sizes, dim3(trk_grid(n)), dim3(256), 0, 0, n, label, d.size);
  hipLaunchKernelGGL(k_tracks_keys, dim3(trk_grid(n)), dim3(256), 0, 0, n, label, d.size, (const unsigned char *)nullptr, d.min_length, d.n_images, d.key);
  tracks_scan(n, d.key, d.scan1, d.sums, d.total);
  MVBA_HIP(hipGetLastError());
  trk_u64 total = 0;
  MVBA_HIP(hipMemcpy(&total, d.total, sizeof(trk_u64), hipMemcpyDeviceToHost));
  d.n_cand = (int)(total >> 32);
  d.n_ent = (int)(unsigned)total;
  if (!d.n_cand) return MVBA_OK;
  if ((rc = d.tmp.alloc(&d.cand, (size_t)d.n_cand)) || (rc = d.tmp.alloc(&d.seg, (size_t)d.n_ent)) || (rc = d.tmp.alloc(&d.sorted, (size_t)d.n_ent)) ||
      (rc = d.tmp.alloc(&d.cam, (size_t)d.n_ent)))
    return rc;
  hipLaunchKernelGGL(k_tracks_cands, dim3(trk_grid(n)), dim3(256), 0, 0, n, d.key, d.scan1, d.cand);
  hipLaunchKernelGGL(k_tracks_fill, dim3(trk_grid(n)), dim3(256), 0, 0, n, label, d.key, d.scan1, d.cursor, d.seg);
  hipLaunchKernelGGL(k_tracks_sort, dim3(trk_grid(d.n_cand)), dim3(256), 0, 0, d.n_cand, d.cand, d.scan1, d.size, d.seg, d.kp, d.n_images, d.sorted, d.cam);
  hipLaunchKernelGGL(k_tracks_conflict, dim3(trk_grid(d.n_ent)), dim3(256), 0, 0, d.n_ent, d.sorted, d.cam, label, d.bad);
  return MVBA_OK;
}

// the survivors numbered (the second scan) and placed: their observations, and every node's track
int tracks_survivors(TracksDev &d, bool want_xy) {
  int rc;
  const int n = d.n;
  const int *label = d.parent;
  hipLaunchKernelGGL(k_tracks_keys, dim3(trk_grid(n)), dim3(256), 0, 0, n, label, d.size, d.bad, d.min_length, d.n_images, d.key);
  tracks_scan(n, d.key, d.scan2, d.sums, d.total + 1);
  MVBA_HIP(hipGetLastError());
  trk_u64 total = 0;
  MVBA_HIP(hipMemcpy(&total, d.total + 1, sizeof(trk_u64), hipMemcpyDeviceToHost));
  d.n_tracks = (int)(total >> 32);
  d.n_obs = (int)(unsigned)total;
  if ((rc = d.tmp.alloc(&d.ptr, (size_t)d.n_tracks + 1)) || (rc = d.tmp.alloc(&d.obs, (size_t)d.n_obs))) return rc;
  if (want_xy && (rc = d.tmp.alloc(&d.xy, (size_t)d.n_obs))) return rc;
  if (d.n_obs)  // (cam_idx into d.seg: the unsorted segments have been read for the last time)
    hipLaunchKernelGGL(k_tracks_out_obs, dim3(trk_grid(d.n_ent)), dim3(256), 0, 0, d.n_ent, d.sorted, d.cam, label, d.bad, d.scan1, d.scan2, d.kpxy, d.obs,
                       d.seg, d.xy);
  hipLaunchKernelGGL(k_tracks_out_nodes, dim3(trk_grid(n)), dim3(256), 0, 0, n, label, d.size, d.bad, d.scan2, d.min_length, d.n_images, d.track, d.ptr, d.cnt);
  return MVBA_OK;
}

// the answer to the caller's arrays; counts [TRK_N_COUNTS] but for the rounds
int tracks_download(const TracksDev &d, int64_t *pt_ptr, int32_t *cam_idx, int32_t *obs_node, double *xy, int32_t *node_track, int64_t *counts) {
  static_assert(sizeof(trk_u64) == sizeof(int64_t) && sizeof(long long) == sizeof(int64_t), "the counters and pt_ptr come back as they are");
  const size_t n_obs = (size_t)d.n_obs;
  MVBA_HIP(hipMemcpy(counts, d.cnt, sizeof(int64_t) * TRK_N_COUNTS, hipMemcpyDeviceToHost));
  counts[TRK_C_TRACKS] = d.n_tracks;
  counts[TRK_C_OBS] = d.n_obs;
  MVBA_HIP(hipMemcpy(node_track, d.track, sizeof(int) * (size_t)d.n, hipMemcpyDeviceToHost));
  if (d.n_tracks) MVBA_HIP(hipMemcpy(pt_ptr, d.ptr, sizeof(int64_t) * (size_t)d.n_tracks, hipMemcpyDeviceToHost));
  pt_ptr[d.n_tracks] = d.n_obs;
  if (n_obs) {
    MVBA_HIP(hipMemcpy(obs_node, d.obs, sizeof(int) * n_obs, hipMemcpyDeviceToHost));
    MVBA_HIP(hipMemcpy(cam_idx, d.seg, sizeof(int) * n_obs, hipMemcpyDeviceToHost));
    if (xy) MVBA_HIP(hipMemcpy(xy, d.xy, sizeof(double2) * n_obs, hipMemcpyDeviceToHost));
  }
  return MVBA_OK;
}

}  // namespace

extern "C" {

int mvba_build_tracks(int32_t n_images, const int64_t *kp_ptr, const double *kp_xy, const int32_t *edges, int64_t n_edges,
                      const uint8_t *edge_ok, int32_t min_length, int64_t *pt_ptr, int32_t *cam_idx, int32_t *obs_node, double *xy,
                      int32_t *node_track, int64_t *counts, double *timings_ms, int32_t device) {
  InitClock clk;  // (the upload lap holds the checks: the pass over the edge ids is most of it)
  int rc = tracks_check_args(n_images, kp_ptr, kp_xy, edges, n_edges, min_length, pt_ptr, cam_idx, obs_node, xy, node_track, counts);
  if (rc) return rc;
  for (int i = 0; i < TRK_N_COUNTS; ++i) counts[i] = 0;
  if (timings_ms) timings_ms[0] = timings_ms[1] = timings_ms[2] = timings_ms[3] = 0.0;
  pt_ptr[0] = 0;
  if (kp_ptr[n_images] == 0) return MVBA_OK;
  if (device >= 0) MVBA_HIP(hipSetDevice(device));
  TracksDev d;
  d.n = (int)kp_ptr[n_images]; d.n_images = n_images; d.min_length = min_length; d.n_edges = n_edges;
  if ((rc = tracks_upload(d, kp_ptr, kp_xy, edges, edge_ok, xy != nullptr))) return rc;
  if (timings_ms) timings_ms[0] = clk.lap();
  EvLaps ev;
  if ((rc = ev.create(3))) return rc;
  int64_t rounds = 0;
  ev.mark();
  if ((rc = tracks_labels(d, &rounds))) return rc;
  ev.mark();
  if ((rc = tracks_candidates(d)) || (rc = tracks_survivors(d, xy != nullptr))) return rc;
  ev.mark();
  MVBA_HIP(hipGetLastError());
  if ((rc = tracks_download(d, pt_ptr, cam_idx, obs_node, xy, node_track, counts))) return rc;
  counts[TRK_C_ROUNDS] = rounds;
  if (timings_ms) {
    timings_ms[1] = ev.ms(0, 1);
    timings_ms[2] = ev.ms(1, 2);
    timings_ms[3] = lap_rest(clk.lap(), timings_ms[1] + timings_ms[2]);
  }
  return MVBA_OK;
}

}  // extern "C"
