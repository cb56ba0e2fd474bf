// Engine creation (mvba_create, mvba_create_robust) -- host code, gfx950.
//
// Included by mvba.hip inside its host-side namespace, after mvba_engine.h: uses its mvba_handle, CreateKnobs and kernel tables
// (resid_jac_kernel, cost_kernel, backsub_kernel, dense_kernel, k1_lds_bytes, cam_lds_bytes), DevBufs and MVBA_HIP.  create_engine() at the end is the
// table of contents; the stages above it stand in the order it calls them:
//
//   validate_problem      argument checks, point of every observation
//   build_k1_tiles        K1's wave tiles and the pieces of points with more than 64 observations
//   k1_block_threads      K1's block size
//   decide_schur_form     THE decision between the dense, slot (21 or 64 lists per wave) and unit forms of K3, with the sub-list sizes and point ranges
//   build_index_host      the pair-major index on host threads (MVBA_INDEX=host)        } both fill one SchurIndex, entry for
//   build_index_device    the same index by the k_idx_* kernels                         } entry the same (tests/test_schur_index*)
//   alloc_engine_buffers, upload_engine, set_kernel_attributes
//
// Device memory: the engine's buffers come from h->mem, the temporaries of creation from a DevBufs on a stage's stack.  A stage
// returns its status; create_engine destroys the half-built handle once.

// mvba_create, xy_layout 1: the observations of a fully visible scene arrive as image planes [m][N] and leave in observation
// order [N][m] (a wave reads 1 KiB of one plane and writes 64 records m * 16 bytes apart; once per engine)
__global__ __launch_bounds__(256) void k_xy_from_planes(const double2 *__restrict__ planes, long long N, int m, double2 *__restrict__ xy) {
  const long long a = (long long)blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y;
  if (a < N) xy[a * m + k] = planes[(long long)k * N + a];
}

#define CR(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

// MVBA_CREATE_TIMING=1: wall time of mvba_create's stages on stderr (tools/time_create.py; the engine's construction is a
// third of the reference's pipeline at 1 M points x 12 images)
struct CreateTimer {
  bool on;
  std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
  void lap(const char *what) {
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "mvba_create: %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now;
  }
};

// ---------------------------------------------------------------- validation, K1
int validate_problem(const mvba_problem *p, std::vector<int> &obs_pt) {
  if (p->n_points < 0 || p->n_images < 2 || p->n_obs < 0 || !p->pt_ptr || (p->n_obs && (!p->cam_idx || !p->xy)))
    return fail(MVBA_ERR_BADARG, "bad problem sizes or null arrays (need n_images >= 2)");
  if (p->gauge_axis != 0 && p->gauge_axis != 1) return fail(MVBA_ERR_BADARG, "gauge_axis must be 0 or 1");
  if (p->xy_layout != 0 && p->xy_layout != 1) return fail(MVBA_ERR_BADARG, "xy_layout must be 0 (observation order) or 1 (image planes)");
  if (p->xy_layout == 1 && p->n_obs != p->n_points * (int64_t)p->n_images)
    return fail(MVBA_ERR_BADARG, "xy as image planes needs every point observed in every image (n_obs = n_points * n_images)");
  // the kernels keep the whole camera table in LDS (K1: 18 doubles per camera + 8 x 8 KiB of wave
  // tiles; back-substitution: 28 per camera): 160 KiB per workgroup caps the camera count.  (The documented limit is
  // round 1's, from 19 doubles per camera; 18 would admit 682.)
  static_assert(LDS_CAMERAS * CAM_LDS + 8 * 64 * 2 * 8 + 2 <= 160 * 1024 / 8 && LDS_CAMERAS * (CAM_LDS + DXI_LDS) <= 160 * 1024 / 8,
                "the camera tables of LDS_CAMERAS cameras fit one workgroup's LDS");
  // (beyond LDS_CAMERAS the same kernels read the tables from device memory -- round 5; what caps the count now is the dense
  // reduced system: D = 9 m - 7 = 36,857 at 4096 cameras is 10.9 GB of matrix, and the unit descriptors keep camera ids in 16 bits)
  constexpr int MAX_CAMERAS = 4096;
  if (p->n_images > MAX_CAMERAS)
    return fail(MVBA_ERR_BADARG, "n_images = " + std::to_string(p->n_images) + " exceeds the " + std::to_string(MAX_CAMERAS) +
                                     " cameras this build solves a dense reduced system for");
  if (p->pt_ptr[0] != 0 || p->pt_ptr[p->n_points] != p->n_obs) return fail(MVBA_ERR_BADARG, "pt_ptr does not span n_obs");
  if (p->n_obs >= (1LL << 31) || p->n_points >= (1LL << 31))
    return fail(MVBA_ERR_BADARG, "n_obs and n_points per handle must be < 2^31");
  const long long N = p->n_points, nobs = p->n_obs;
  const int m = p->n_images;
  // validate + build point-of-observation
  obs_pt.resize(nobs);
  for (long long a = 0; a < N; ++a) {
    const long long o0 = p->pt_ptr[a], o1 = p->pt_ptr[a + 1];
    if (o1 < o0 || o1 > nobs) return fail(MVBA_ERR_BADARG, "pt_ptr not monotone / out of range");
    for (long long o = o0; o < o1; ++o) {
      const int k = p->cam_idx[o];
      if (k < 0 || k >= m) return fail(MVBA_ERR_BADARG, "cam_idx out of range");
      if (o > o0 && p->cam_idx[o - 1] >= k) return fail(MVBA_ERR_BADARG, "cam_idx must ascend within a point");
      obs_pt[o] = (int)a;
    }
  }
  return MVBA_OK;
}

// K1 wave tiles: whole points packed greedily into <= 64 observations; a point with more than
// 64 observations is cut into pieces whose tiles are flagged by a complemented (negative) start
struct K1Tiles {
  std::vector<int> tiles, tile_slot;
  std::vector<int4> splits;
  int n_split_slots = 0;
  bool any_split = false;
};

K1Tiles build_k1_tiles(const mvba_problem *p) {
  K1Tiles t;
  const long long N = p->n_points;
  long long cur0 = 0, fill = 0;
  auto flush = [&](bool split_flag) { t.tiles.push_back(split_flag ? ~(int)cur0 : (int)cur0); };
  for (long long a = 0; a < N; ++a) {
    const long long d = p->pt_ptr[a + 1] - p->pt_ptr[a];
    if (d > 64) {
      if (fill) { flush(false); cur0 += fill; fill = 0; }
      t.any_split = true;
      t.splits.push_back(make_int4((int)a, t.n_split_slots, (int)((d + 63) / 64), 0));
      for (long long q = 0; q < d; q += 64) {
        t.tile_slot.resize(t.tiles.size() + 1, -1);
        t.tile_slot[t.tiles.size()] = t.n_split_slots++;
        flush(true);
        cur0 += std::min<long long>(64, d - q);
      }
      continue;
    }
    if (fill + d > 64) { flush(false); cur0 += fill; fill = 0; }
    fill += d;
  }
  if (fill) { flush(false); cur0 += fill; }
  t.tiles.push_back((int)p->n_obs);  // terminator (never negative: only its magnitude is used)
  return t;
}

// K1: the waves of a block share one camera table in LDS and bring 8 KiB of staging each.  Up to ~100 cameras two blocks
// of 8 waves fill a CU (16 waves: the register limit); beyond that ONE block fits and its size decides the occupancy --
// the smallest block that reaches the most waves per CU (200 cameras: 16 waves, 0.96 -> 0.70 ms at 1 M points x 10 %;
// 300: 14, 0.41 -> 0.32-0.37; 500: 11, config 4's shard 1.53-1.58 -> 1.32-1.36)
int k1_block_threads(int m, bool gcam) {
  int best_w = 8, best_tot = 0;
  for (int w = 8; w <= 16; ++w) {
    const size_t per = k1_lds_bytes(m, gcam, 64 * w);
    if (per > 160 * 1024) break;
    const int tot = std::min<int>(16, (int)(160 * 1024 / per) * w);
    if (tot > best_tot) { best_tot = tot; best_w = w; }
  }
  return 64 * best_w;
}

// ---------------------------------------------------------------- what the two index builders share
// ---- pair-major Schur index (see k_schur_pairs).  Items (obs of k, obs of l, point) for every
// pair k <= l of a point's cameras, counting-sorted by pair, ascending point inside a pair.
inline long long pair_id(int m, int k, int l) { return (long long)k * m - (long long)k * (k - 1) / 2 + (l - k); }

// Both passes of the host build over the points run on host threads that OWN strips (camera k belongs to thread
// k % n_thr): every thread scans the whole observation list but touches only its own pairs, so
// there is nothing to lock and the order inside a pair's list stays ascending by point.
template <typename F>
void on_threads(int n_thr, F body) {
  std::vector<std::thread> th;
  for (int t = 1; t < n_thr; ++t) th.emplace_back(body, t);
  body(0);
  for (auto &x : th) x.join();
}

// what every stage of the index reads: the problem, the device copy of its topology, the stream
struct IndexInput {
  const mvba_problem *p;
  long long N, nobs, P;  // P pairs k <= l
  int m, n_thr;          // host threads (at most 16, at most one per camera)
  hipStream_t stream;
  const long long *d_pt_ptr;
  const int *d_cam;
};

// The lists: pair q is dealt round-robin into S[q] sub-lists, list v = vp_ptr[q] + sub-list holds items vp_off[v] .. vp_off[v + 1]
struct PairLists {
  std::vector<long long> cnt;  // items per pair
  long long T = 0, Tdiag = 0;  // items in all, in the diagonal pairs
  long long target = 1;        // the typical off-diagonal pair
  long long unit_items = 600;  // items per unit of the unit form
  std::vector<int> S, vp_ptr;
  int VP = 0;
  std::vector<long long> vp_off;
  long long n_diag_lists = 0, n_off_lists = 0;
  // slot form: waves (of W lists) per range, diagonal + off-diagonal
  long long slot_waves(int W) const { return (n_diag_lists + W - 1) / W + (n_off_lists + W - 1) / W; }
};

int size_pair_lists(const IndexInput &in, PairLists &L) {
  const int m = in.m;
  const long long P = in.P, N = in.N;
  for (int k = 0; k < m; ++k) L.Tdiag += L.cnt[pair_id(m, k, k)];
  for (long long q = 0; q < P; ++q) L.T += L.cnt[q];
  if (L.T >= (1LL << 40)) return fail(MVBA_ERR_BADARG, "too many (point, camera pair) items");
  const long long T = L.T, Tdiag = L.Tdiag;
  // a pair much larger than the typical off-diagonal one (the diagonal pairs: every observation of
  // the camera) is dealt round-robin into S sub-lists that sweep the points at the common pace
  L.target = std::max<long long>(1, (T - Tdiag) / std::max<long long>(1, P - m));
  // items per unit (a wave's run): shorter units keep the sibling units of a strip closer together in time (more L2
  // hits on the k side) but cost a serial prologue and a 27-value tree each.  With one-wave blocks and static
  // assignment the best length is ~600 (config 3: 1.99 / 1.86 / 1.80 / 1.81 / 1.89 / 2.03 ms at 320 / 448 / 576 /
  // 640 / 768 / 1024; with four-wave blocks and atomic queues it was 768)
  // Round 4, re-swept where the unit form actually runs (beyond one round of the slot form): the sparser the pairs, the longer
  // the stretch of points a unit of U items spans (U / p^2) and the further its siblings drift apart -- config 4's shard (5 %):
  // 14.40 / 13.89 / 13.99 / 14.49 / 15.6 ms at 600 / 400 / 300 / 250 / 200 (L2 misses 743 M -> 553 M at 300, the per-unit
  // prologue and tree eat the rest); 1 M x 200 x 10 %: 6.21 / 6.61 / 7.12 at 600 / 400 / 300; 300 k x 300 x 5 %: 1.37 / 1.23 / 1.23
  // (profiles/r04_sweep_pairs_unit.txt).  So: 600 at one item per pair per 100 points, 400 at one per 400.
  // (Two gathers in flight -- this form on the slot kernel's ring loop -- make it SLOWER, 15.5 ms: the wider window of
  // points misses L2 more often, profiles/r04_sweep_pairs_ring.txt.)
  const double pair_rate = N > 0 && P > m ? (double)(T - Tdiag) / ((double)(P - m) * (double)N) : 0.01;
  L.unit_items = (long long)std::max(300.0, std::min(600.0, 200.0 + 4000.0 * std::sqrt(pair_rate)));
  L.S.resize(P);
  L.vp_ptr.assign(P + 1, 0);
  for (long long q = 0; q < P; ++q) {
    L.S[q] = (int)std::max<long long>(1, std::min<long long>(256, (L.cnt[q] + L.target / 2) / L.target));
    L.vp_ptr[q + 1] = L.vp_ptr[q] + L.S[q];
  }
  L.VP = L.vp_ptr[P];
  for (int k = 0; k < m; ++k) {
    L.n_diag_lists += L.S[pair_id(m, k, k)];
    for (int l = k + 1; l < m; ++l) L.n_off_lists += L.S[pair_id(m, k, l)];
  }
  // The points are swept in their natural order: an item's key (where its point sits in the sweep, in observations) is its
  // point's first observation, pt_ptr[a].  (A low-discrepancy order -- round 4 -- cut the padding rows from 12.4 % to 10.4 %
  // at config 3 but k_schur_slots only from 1.691 to 1.677 ms, for 0.12 s more of mvba_create: profiles/r04_sweep_point_order.txt.)
  L.vp_off.assign(L.VP + 1, 0);
  for (long long q = 0; q < P; ++q)
    for (int sI = 0; sI < L.S[q]; ++sI) L.vp_off[L.vp_ptr[q] + sI + 1] = (L.cnt[q] - sI + L.S[q] - 1) / L.S[q];
  for (int v = 0; v < L.VP; ++v) L.vp_off[v + 1] += L.vp_off[v];
  return MVBA_OK;
}

// point ranges.  Unit form: long runs for big problems, but small ones still get ~4096 units of >= 128 items.
// Slot form: 8 ranges (one per XCD) -- 8 j while j ranges' worth of waves fit an XCD and a list keeps >= 64 items.  The lane form
// (W = 64, not paced) takes `lane_nR` ranges instead: lane_ranges (mvba_engine_host.h), counted from the chip's wave places, any
// number from 1 on; which block runs wave w of range r is the kernel's affair (lane_wave_of_block keeps a range on one XCD).
struct PointRanges {
  int nR = 1;
  std::vector<long long> lo;  // [nR + 1] first point of every range
};

PointRanges make_ranges(const IndexInput &in, const PairLists &L, bool slots, int xcd_waves, int W, int lane_nR = 0) {
  PointRanges R;
  const long long N = in.N;
  if (slots) {
    const long long j = std::max<long long>(1, std::min<long long>(xcd_waves / std::max(1LL, L.slot_waves(W)), L.target / (8 * 64)));
    R.nR = W == LANES_W ? std::max(1, lane_nR) : (int)(8 * std::min<long long>(j, 8));
    R.lo.assign(R.nR + 1, 0);
    // equal ITEM counts: the ranges run side by side
    std::vector<long long> pre(N + 1, 0);
    for (long long a = 0; a < N; ++a) {
      const long long d = in.p->pt_ptr[a + 1] - in.p->pt_ptr[a];
      pre[a + 1] = pre[a] + d * (d + 1) / 2;
    }
    for (int r = 0; r <= R.nR; ++r)
      R.lo[r] = std::lower_bound(pre.begin(), pre.end(), (long long)((__int128)pre[N] * r / R.nR)) - pre.begin();
    R.lo[0] = 0; R.lo[R.nR] = N;
  } else {
    const long long nR_big = (L.target + L.unit_items / 2) / L.unit_items, nR_fill = std::min<long long>((4096 + L.VP - 1) / L.VP, L.target / 128);
    R.nR = (int)std::max<long long>(1, std::min<long long>(64, std::max(nR_big, nR_fill)));
    R.lo.assign(R.nR + 1, 0);
    for (int r = 0; r <= R.nR; ++r) R.lo[r] = (long long)((__int128)N * r / R.nR);
  }
  return R;
}

// Tuning of the slot form with one lane per item (k_schur_lanes), measured at config 3 and on its camera sweep (DESIGN.md §3.1,
// profiles/r06_lanes_product.txt)
constexpr long long LANES_SKEW = 12288;     // bounded skew of its step merge over 64 slots (twice that: fewer padding rows, slower)
// taken by mvba_create itself from this many waves per point range on.  With the ranges counted by wave places (lane_ranges) a
// short range no longer leaves places empty: 1 M points x 10 %, k_schur_lanes_compact against k_schur_slots, 60 cameras (38 waves,
// 26 ranges) 0.61 against 0.74 ms, 70: 0.74 / 1.05, 80 (63 waves, 16 ranges): 0.86 / 1.13, 90 (78, 13): 1.08 / 1.39, 100 (95, 10):
// 1.30 / 1.57 (profiles/r09_lanes_four_waves.txt; with 8 j ranges and three waves per CU it was 78: 80 cameras lost 1.32 to 1.19).
// Below 60 cameras nothing was measured: the bound is the smallest scene that was.  (MVBA_REC=full, an A/B knob, shares it.)
constexpr long long LANES_MIN_WAVES = 38;

// What decide_schur_form answers: the form, and for the pair-major forms the lists and ranges the index is built from
struct SchurPlan {
  int mode = SCHUR_SLOTS;
  int W = PSTEP;               // SCHUR_SLOTS: lists per wave = items per step (PSTEP: k_schur_slots, LANES_W: k_schur_lanes)
  std::vector<int> dense_obs;  // SCHUR_DENSE with missing observations: [N][m] observation of (point, camera) or -1
  PairLists L;
  PointRanges R;
  int lane_places = 0;         // W = LANES_W: waves of the lane kernel per CU (the occupancy query's answer) the ranges were counted from
};

// THE decision of K3's form; the only place that names a form as the engine's.  `count_pairs(cnt)` runs the counting pass of
// the index build that create_engine chose (host threads or device): the pair-major forms are told apart by what it finds.
template <typename CountPairs>
int decide_schur_form(const IndexInput &in, const CreateKnobs &knobs, int loss, bool compact_rec, int device, CountPairs count_pairs,
                      SchurPlan &plan, CreateTimer &timer) {
  const mvba_problem *p = in.p;
  const long long N = in.N, nobs = in.nobs;
  const int m = in.m;
  {  // up to 21 cameras and most (point, camera) pairs observed: the dense form (no pair index).  Full visibility in camera order
     // (the reference's own scenes): a point's records are read as one contiguous range; otherwise through a table, a missing
     // observation standing as a zero record (the matrix cores multiply the zeros: worth it from ~60 % visibility on)
    bool few = m >= 1 && 9 * m <= 16 * DENSE_MAX_TILES && N > 0, full = few && nobs == N * (long long)m;
    for (long long a = 0; a < N && full; ++a) {
      if (p->pt_ptr[a + 1] - p->pt_ptr[a] != m) { full = false; break; }
      const int *ci = p->cam_idx + p->pt_ptr[a];
      for (int k = 0; k < m; ++k)
        if (ci[k] != k) { full = false; break; }
    }
    const bool forced = knobs.schur_dense;
    bool masked = few && !full && (forced || (!knobs.schur_set && (double)nobs >= 0.6 * (double)N * m)) && (long long)N * m < (1LL << 31);
    if (masked) {
      plan.dense_obs.assign((size_t)N * m, -1);
      for (long long a = 0; a < N && masked; ++a)
        for (long long o = p->pt_ptr[a]; o < p->pt_ptr[a + 1]; ++o) {
          int &slot = plan.dense_obs[(size_t)a * m + p->cam_idx[o]];
          if (slot >= 0) { masked = false; break; }  // (a camera twice in one point: the pair-major forms take such scenes)
          slot = (int)o;
        }
      if (!masked) plan.dense_obs.clear();
    }
    timer.lap("form of K3");
    if ((full && (!knobs.schur_set || forced)) || masked) {
      plan.mode = SCHUR_DENSE;
      return MVBA_OK;
    }
  }
  plan.L.cnt.assign(in.P, 0);
  CR(count_pairs(plan.L.cnt));
  timer.lap("pair counts");
  CR(size_pair_lists(in, plan.L));
  const PairLists &L = plan.L;
  // ---- which form of the kernel: the slot-resident one (k_schur_slots) needs all lists that sweep a point range
  // TOGETHER resident on one XCD at once -- 9 waves per CU (LDS) x n_cu / 8 CUs x 21 slots = 6048 lists.  Up to ~100
  // cameras at 10 % visibility (4950 pairs + ~1000 sub-lists of the diagonal pairs) that is every list.  Beyond that
  // the engine takes the unit form (cutting the cameras into groups swept in rounds lost to it on every workload
  // measured: DESIGN.md 3.1, "Round 4").  The same form with one lane per item (k_schur_lanes, 64 lists per wave) has
  // 3 waves per CU: 96 waves = 6144 lists per XCD.
  int n_cu_dev = 256;
  hipDeviceGetAttribute(&n_cu_dev, hipDeviceAttributeMultiprocessorCount, device);
  auto xcd_waves = [&](int W) { return std::max(1, n_cu_dev / 8) * (W == LANES_W ? 160 * 1024 / LANES_LDS : 160 * 1024 / SLOT_LDS); };
  // (below ~4 M items the launch is all prologue and pacing: the unit form's many short waves win -- config 2,
  // 10k points x 20 cameras: 0.095 against 0.124 ms; equal at 5.5 M items; MVBA_SCHUR=slots | lanes keeps the slot form)
  const bool slots_forced = knobs.schur_slots || knobs.schur_lanes;
  // (a robust loss never takes the slot form: the unit form then, as when the lists do not fit one round -- DESIGN.md §12)
  // (the gathers use 32-bit byte offsets: point rows from the array's start, records from their RANGE's first
  // observation -- the latter checked per plan, once the ranges are known)
  const bool may_slots = !knobs.schur_pairs && loss == LOSS_SQUARED && (N + 1) * 128LL < (1LL << 32) && !knobs.force_big && (L.T >= 4000000 || slots_forced);
  // The lane form's ranges are counted from the wave places of the kernel it will launch (`compact_rec`: k_schur_lanes_compact, four
  // waves of 40 KiB per CU; else k_schur_lanes, three) as the RUNTIME counts them.  What it admits stays a range of 96 waves.
  int lane_places = 0;
  if (may_slots)
    MVBA_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&lane_places, compact_rec ? (const void *)k_schur_lanes_compact : (const void *)k_schur_lanes, 64,
                                                          compact_rec ? LANES_LDS_C : LANES_LDS));
  lane_places = std::max(1, lane_places);
  plan.lane_places = lane_places;
  long long max_degree = 0;
  for (long long a = 0; a < N; ++a) max_degree = std::max<long long>(max_degree, p->pt_ptr[a + 1] - p->pt_ptr[a]);
  // the slot form at W lists per wave: its point ranges, or false where it may not run
  auto slot_plan = [&](int W, PointRanges &R) {
    if (!may_slots || L.slot_waves(W) > xcd_waves(W)) return false;
    R = make_ranges(in, L, true, xcd_waves(W), W,
                    lane_ranges((long long)n_cu_dev * lane_places, L.slot_waves(LANES_W), L.target, knobs.slot_ranges));
    // (few cameras with dense visibility: a dozen cameras are 78 lists = 5 waves per range, 320 waves on the whole chip even with 64
    // ranges -- 1 M points x 12 cameras, all visible: 9.3 ms against 4.9 for the unit form; at 20 cameras, 704 waves, the slot form is
    // ahead again, 9.8 against 10.8: profiles/r05_sweep_few_cameras.txt)
    if (W == PSTEP && !slots_forced && R.nR * L.slot_waves(W) < 512) return false;
    long long widest = 0;
    for (int r = 0; r < R.nR; ++r) widest = std::max<long long>(widest, p->pt_ptr[R.lo[r + 1]] - p->pt_ptr[R.lo[r]]);
    if ((widest + 1) * 128LL >= (1LL << 32)) return false;  // (a range's records span 4 GiB: the unit form's 64-bit-offset build)
    // (W = 64: an item is two packed words -- a point seen more than 16,384 times does not pack: k_schur_slots, then the unit form)
    return W != LANES_W || lane_idx_fits(N, widest, max_degree);
  };
  // The slot form first where it may run, else the unit form.  One lane per item (W = 64) by itself only where k_schur_slots
  // would run too and a range has LANES_MIN_WAVES .. 96 waves of 64 lists; MVBA_SCHUR=lanes asks for it wherever its own
  // capacity holds and falls back to k_schur_slots, then to the unit form; MVBA_SCHUR=slots keeps k_schur_slots.
  PointRanges R21, R64;
  const bool fits21 = slot_plan(PSTEP, R21);
  const bool lanes = knobs.schur_lanes ? slot_plan(LANES_W, R64)
                                       : (fits21 && !knobs.schur_slots && L.slot_waves(LANES_W) >= LANES_MIN_WAVES && slot_plan(LANES_W, R64));
  if (lanes) {
    plan.mode = SCHUR_SLOTS; plan.W = LANES_W; plan.R = std::move(R64);
  } else if (fits21) {
    plan.mode = SCHUR_SLOTS; plan.W = PSTEP; plan.R = std::move(R21);
  } else {
    plan.mode = SCHUR_PAIRS;
    plan.R = make_ranges(in, L, false, 0, PSTEP);
  }
  return MVBA_OK;
}

// The pair-major index as the engine takes it.  Host arrays, except the items of a device build: those are already where the
// kernels read them (d_it_*, d_seg_end: buffers of the engine) and the host vectors stay empty.
struct SchurIndex {
  std::vector<int> it_k, it_l, it_a;  // items: pair-major (unit form) or step-major with padding rows (slot form)
  std::vector<int4> units;            // (first item lo, hi, items, k << 16 | l), numbered pair-major
  std::vector<int> unit_ptr;          // [P + 1] first unit of every pair
  std::vector<int> q_ptr = std::vector<int>(9, 0), q_units;  // unit form: the work queue of every XCD
  std::vector<int4> wdesc;            // slot form: (first step lo, hi, steps, flags) per wave
  std::vector<int> wunits, seg_end;   // ... its W units, and the steps taken at the end of every pacing segment
  long long n_items = 0, n_items_offdiag = 0, n_slot_items = 0;  // what mvba_get_info reports
  int n_waves = 0, slot_nR = 8, slot_nseg = 0, slot_w = PSTEP;
  bool on_device = false;
  int *d_it_k = nullptr, *d_it_l = nullptr, *d_it_a = nullptr, *d_seg_end = nullptr;
  long long *d_range_o0 = nullptr;    // slot form: first observation of every range
};

// units: (pair, sub-list, point range), numbered pair-major (k_schur_reduce sums them in this order).  bound(v, r) is the first
// item of list v at or after the first point of range r.  uid[v * nR + r]: the unit of list v in range r, or -1.
template <typename Bound>
void number_units(const IndexInput &in, const SchurPlan &plan, Bound bound, SchurIndex &ix, std::vector<int> &uid) {
  const int m = in.m, nR = plan.R.nR;
  const PairLists &L = plan.L;
  ix.unit_ptr.assign(in.P + 1, 0);
  uid.assign((size_t)L.VP * nR, -1);
  for (int k = 0; k < m; ++k)
    for (int l = k; l < m; ++l) {
      const long long q = pair_id(m, k, l);
      ix.unit_ptr[q] = (int)ix.units.size();
      for (int sI = 0; sI < L.S[q]; ++sI) {
        const int v = L.vp_ptr[q] + sI;
        for (int r = 0; r < nR; ++r) {
          const long long lo = bound(v, r), hi = bound(v, r + 1);
          if (hi <= lo) continue;
          uid[(size_t)v * nR + r] = (int)ix.units.size();
          ix.units.push_back(make_int4((int)(lo & 0xffffffffLL), (int)(lo >> 32), (int)(hi - lo), (k << 16) | l));
        }
      }
    }
  ix.unit_ptr[in.P] = (int)ix.units.size();
}

// work queues: strip k on XCD k % 8, inside a queue by (range, k, l, sub-list) -- range-major: every XCD sweeps the
// point ranges in the same order, so the l-side records of a range (needed once per strip, ~4.5 times in all) are
// re-read from the Infinity Cache while the whole chip is on that range: 2.28 -> 2.04 ms at config 3 against strip-major
void build_work_queues(const IndexInput &in, const SchurPlan &plan, const std::vector<int> &uid, SchurIndex &ix) {
  const int m = in.m, nR = plan.R.nR;
  const PairLists &L = plan.L;
  for (int x = 0; x < 8; ++x) {
    auto push_group = [&](int k, int r) {
      for (int l = k; l < m; ++l) {
        const long long q = pair_id(m, k, l);
        for (int sI = 0; sI < L.S[q]; ++sI) {
          const int id = uid[(size_t)(L.vp_ptr[q] + sI) * nR + r];
          if (id >= 0) ix.q_units.push_back(id);
        }
      }
    };
    for (int r = 0; r < nR; ++r)
      for (int k = x; k < m; k += 8) push_group(k, r);
    ix.q_ptr[x + 1] = (int)ix.q_units.size();
  }
}

// Tuning of the slot form's host-built schedule (k_schur_slots), in observations of a point range
constexpr long long SLOT_SKEW = 12288;  // bounded skew of the step merge
constexpr long long SLOT_SEG = 8192;    // pacing segment
constexpr int SLOT_LAG = 4;             // a wave enters segment j only when all waves of its range have left segment j - lag
constexpr long long slot_skew(int W) { return W == LANES_W ? LANES_SKEW : SLOT_SKEW; }

// The slot form's waves: block b = nR w + r is wave w of range r and runs on XCD r % 8 (the lane form: WAVE b, run by the block
// lane_wave_of_block assigns it).  sl_beg / sl_len: the span of items
// each of its 21 slots merges (from the units); w_steps / w_beg: the steps it takes and its first step, once merged.
struct SlotWaves {
  long long n_waves = 0;
  int nSeg = 1;
  std::vector<int> w_isdiag;  // per wave of a range
  std::vector<long long> sl_beg, w_steps, w_beg;
  std::vector<int> sl_len;
};

// ---- waves of W = 21 (64: k_schur_lanes, whose nR need not be a multiple of 8) lists, every wave once per range; the diagonal pairs'
// sub-lists come FIRST: a CU's SIMDs
// arbitrate by age, the blocks dispatched last share a SIMD three ways as its youngest wave and fall behind --
// and a diagonal step is the dearer one
SlotWaves make_slot_waves(const IndexInput &in, const SchurPlan &plan, const std::vector<int> &uid, SchurIndex &ix) {
  const int m = in.m, nR = plan.R.nR;
  const PairLists &L = plan.L;
  const int W = plan.W;
  SlotWaves sw;
  std::vector<int> wl;  // [wave of a range][W] list ids v = vp_ptr[pair] + sub-list, -1: none
  std::vector<int> diag_lists, off_lists;
  for (int k = 0; k < m; ++k) {
    for (int sI = 0; sI < L.S[pair_id(m, k, k)]; ++sI) diag_lists.push_back(L.vp_ptr[pair_id(m, k, k)] + sI);
    for (int l = k + 1; l < m; ++l)
      for (int sI = 0; sI < L.S[pair_id(m, k, l)]; ++sI) off_lists.push_back(L.vp_ptr[pair_id(m, k, l)] + sI);
  }
  for (const std::vector<int> *src : {&diag_lists, &off_lists})
    for (size_t first = 0; first < src->size(); first += W) {
      for (int sl = 0; sl < W; ++sl) wl.push_back(first + sl < src->size() ? (*src)[first + sl] : -1);
      sw.w_isdiag.push_back(src == &diag_lists);
    }
  const long long n_waves = sw.n_waves = (long long)sw.w_isdiag.size() * nR;
  ix.wdesc.assign(n_waves, make_int4(0, 0, 0, 0));
  ix.wunits.assign((size_t)n_waves * W, -1);
  sw.w_steps.assign(n_waves, 0);
  sw.w_beg.assign(n_waves + 1, 0);
  sw.sl_beg.assign((size_t)n_waves * W, 0);
  sw.sl_len.assign((size_t)n_waves * W, 0);
  for (long long b = 0; b < n_waves; ++b) {
    const int *vs = wl.data() + (size_t)(b / nR) * W;
    const int r = (int)(b % nR);
    for (int sl = 0; sl < W; ++sl) {
      const int id = vs[sl] >= 0 ? uid[(size_t)vs[sl] * nR + r] : -1;
      ix.wunits[(size_t)b * W + sl] = id;
      if (id < 0) continue;
      sw.sl_beg[(size_t)b * W + sl] = ((long long)ix.units[id].y << 32) | (unsigned)ix.units[id].x;
      sw.sl_len[(size_t)b * W + sl] = ix.units[id].z;
    }
  }
  // pacing segments: seg_end[b][j] = steps wave b has taken when its slowest slot leaves segment j of the range
  for (int r = 0; r < nR; ++r)
    sw.nSeg = std::max<long long>(sw.nSeg, (in.p->pt_ptr[plan.R.lo[r + 1]] - in.p->pt_ptr[plan.R.lo[r]] + SLOT_SEG - 1) / SLOT_SEG);
  ix.seg_end.assign((size_t)n_waves * sw.nSeg, 0);
  ix.slot_nseg = sw.nSeg;
  return sw;
}

// first observation of every range: the merge kernels and k_schur_slots (its record base) read it
int upload_range_o0(const IndexInput &in, const PointRanges &R, DevBufs &engine, SchurIndex &ix) {
  std::vector<long long> ro0(R.nR);
  for (int r = 0; r < R.nR; ++r) ro0[r] = in.p->pt_ptr[R.lo[r]];
  CR(engine.alloc(&ix.d_range_o0, (size_t)R.nR));
  MVBA_HIP(hipMemcpy(ix.d_range_o0, ro0.data(), sizeof(long long) * R.nR, hipMemcpyHostToDevice));
  return MVBA_OK;
}

// the waves' first steps from their step counts; the size of the step-major index against what the device has
int place_slot_steps(const SchurPlan &plan, SlotWaves &sw, const SchurIndex &ix, long long &total_steps) {
  const int W = plan.W;
  for (long long b = 0; b < sw.n_waves; ++b) sw.w_beg[b + 1] = sw.w_beg[b] + sw.w_steps[b];
  total_steps = sw.w_beg[sw.n_waves];
  if (total_steps * W >= (1LL << 40)) return fail(MVBA_ERR_BADARG, "too many (point, camera pair) items");
  // the step-major index -- its size follows the padding rows -- against the memory that is
  // there, BEFORE anything of it is allocated: three 4-byte arrays of step rows, then the interleaved 256-byte rows beside them
  const size_t need = (size_t)total_steps * W * 12 + (size_t)total_steps * slot_idx_ints(W) * 4 + ix.seg_end.size() * 4;
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) == hipSuccess && need > fr)
    return fail(MVBA_ERR_BADARG, "the slot-form Schur index needs " + std::to_string(need >> 20) + " MiB (" + std::to_string(total_steps * W) + " step rows for " +
                                     std::to_string(plan.L.T) + " items: " + std::to_string(plan.R.nR) + " ranges, skew " + std::to_string(slot_skew(W)) + "), " +
                                     std::to_string(fr >> 20) + " MiB of device memory are free: use MVBA_SCHUR=pairs");
  return MVBA_OK;
}

void finish_slot_waves(const SchurPlan &plan, const SlotWaves &sw, long long total_steps, SchurIndex &ix) {
  const int nR = plan.R.nR, W = plan.W;
  std::vector<int> live(nR, 0);  // waves of a range that run at all: what a pacing counter has to reach
  for (long long b = 0; b < sw.n_waves; ++b) live[b % nR] += sw.w_steps[b] > 0;
  for (long long b = 0; b < sw.n_waves; ++b) {
    const long long beg = sw.w_beg[b];  // first step of the wave in the step-major index
    // flags: bit 0 diagonal wave | bits 8..19 live waves of its range
    ix.wdesc[b] = make_int4((int)(beg & 0xffffffffLL), (int)(beg >> 32), (int)sw.w_steps[b],
                            (sw.w_isdiag[b / nR] ? 1 : 0) | (live[b % nR] << 8));
  }
  ix.n_waves = (int)sw.n_waves;
  ix.slot_nR = nR;
  ix.n_slot_items = total_steps * W;
  ix.slot_w = W;
}

// ---------------------------------------------------------------- the index on host threads (MVBA_INDEX=host)
int count_pairs_host(const IndexInput &in, std::vector<long long> &cnt) {
  const mvba_problem *p = in.p;
  const int m = in.m, n_thr = in.n_thr;
  on_threads(n_thr, [&](int tid) {
    for (long long a = 0; a < in.N; ++a) {
      const int *cb = p->cam_idx + p->pt_ptr[a];
      const int d = (int)(p->pt_ptr[a + 1] - p->pt_ptr[a]);
      for (int i = 0; i < d; ++i) {
        if (cb[i] % n_thr != tid) continue;
        long long *row = cnt.data() + pair_id(m, cb[i], cb[i]) - cb[i];  // row[l] = cnt[pair(k, l)]
        for (int j = i; j < d; ++j) row[cb[j]]++;
      }
    }
  });
  return MVBA_OK;
}

int build_index_host(const IndexInput &in, const SchurPlan &plan, DevBufs &engine, SchurIndex &ix, CreateTimer &timer) {
  const mvba_problem *p = in.p;
  const PairLists &L = plan.L;
  const PointRanges &R = plan.R;
  const long long N = in.N, P = in.P;
  const int m = in.m, n_thr = in.n_thr, nR = R.nR;
  std::vector<int> &it_k = ix.it_k, &it_l = ix.it_l, &it_a = ix.it_a;
  it_k.resize(L.T); it_l.resize(L.T); it_a.resize(L.T);
  {
    std::vector<long long> run(P, 0);
    on_threads(n_thr, [&](int tid) {
      for (long long a = 0; a < N; ++a) {
        const long long o0 = p->pt_ptr[a];
        const int *cb = p->cam_idx + o0;
        const int d = (int)(p->pt_ptr[a + 1] - o0);
        for (int i = 0; i < d; ++i) {
          if (cb[i] % n_thr != tid) continue;
          const long long rowp = pair_id(m, cb[i], cb[i]) - cb[i];
          for (int j = i; j < d; ++j) {
            const long long q = rowp + cb[j], r = run[q]++;
            const int sI = (int)(r % L.S[q]);
            const long long pos = L.vp_off[L.vp_ptr[q] + sI] + r / L.S[q];
            it_k[pos] = (int)(o0 + i); it_l[pos] = (int)(o0 + j); it_a[pos] = (int)a;
          }
        }
      }
    });
  }
  timer.lap("items sorted by pair");
  std::vector<int> uid;
  number_units(in, plan, [&](int v, int r) {
    auto before = [](int a, long long key) { return (long long)a < key; };
    return (long long)(std::lower_bound(it_a.data() + L.vp_off[v], it_a.data() + L.vp_off[v + 1], R.lo[r], before) - it_a.data());
  }, ix, uid);
  timer.lap("units");
  if (plan.mode == SCHUR_SLOTS) {
    SlotWaves sw = make_slot_waves(in, plan, uid, ix);
    const int nSeg = sw.nSeg, W = plan.W;
    const long long skew = slot_skew(W);
    static_assert(PSTEP <= LANES_W, "the merge's cursors");
    std::vector<int> st_k, st_l, st_a;
    // Bounded-skew merge of a wave's lists into steps (see k_schur_slots)
    auto merge = [&](long long b, long long base, bool fill) {
      const int r = (int)(b % nR);
      long long cur[LANES_W], end[LANES_W];
      for (int sl = 0; sl < W; ++sl) {
        cur[sl] = sw.sl_beg[(size_t)b * W + sl];
        end[sl] = cur[sl] + sw.sl_len[(size_t)b * W + sl];
      }
      long long steps = 0;
      const long long o_lo = p->pt_ptr[R.lo[r]];
      int sg = 0;
      auto key_of = [&](int sl) { return p->pt_ptr[it_a[cur[sl]]]; };  // where the item's point sits in the sweep, in observations
      while (true) {
        long long lo = -1;
        for (int sl = 0; sl < W; ++sl)
          if (cur[sl] < end[sl] && (lo < 0 || key_of(sl) < lo)) lo = key_of(sl);
        if (fill && lo >= 0)
          while (sg < nSeg && lo >= o_lo + (sg + 1) * SLOT_SEG) ix.seg_end[(size_t)b * nSeg + sg++] = (int)steps;
        if (lo < 0) break;
        for (int sl = 0; sl < W; ++sl) {
          const bool take = cur[sl] < end[sl] && key_of(sl) <= lo + skew;
          if (fill) {
            const long long o = (base + steps) * W + sl;
            if (take) { st_k[o] = (int)(it_k[cur[sl]] - o_lo); st_l[o] = (int)(it_l[cur[sl]] - o_lo); st_a[o] = it_a[cur[sl]]; }
            else { st_k[o] = st_l[o] = 0; st_a[o] = (int)N; }  // the range's first record (any finite one) x the all-zero point row
          }
          if (take) ++cur[sl];
        }
        ++steps;
      }
      if (fill)
        while (sg < nSeg) ix.seg_end[(size_t)b * nSeg + sg++] = (int)steps;
      return steps;
    };
    CR(upload_range_o0(in, R, engine, ix));
    on_threads(n_thr, [&](int tid) {
      for (long long b = tid; b < sw.n_waves; b += n_thr) sw.w_steps[b] = merge(b, 0, false);
    });
    timer.lap("slot merge (count)");
    long long total_steps = 0;
    CR(place_slot_steps(plan, sw, ix, total_steps));
    st_k.resize(total_steps * W); st_l.resize(total_steps * W); st_a.resize(total_steps * W);
    on_threads(n_thr, [&](int tid) {
      for (long long b = tid; b < sw.n_waves; b += n_thr)
        if (sw.w_steps[b]) merge(b, sw.w_beg[b], true);
    });
    timer.lap("slot merge (fill)");
    finish_slot_waves(plan, sw, total_steps, ix);
    it_k.swap(st_k); it_l.swap(st_l); it_a.swap(st_a);  // what is uploaded: the step-major arrays
  } else {
    build_work_queues(in, plan, uid, ix);
  }
  return MVBA_OK;
}

// ---------------------------------------------------------------- the index on the device (k_idx_*)
// A stable counting sort by pair, every wave walking its own chunk of points with a private pair histogram -- in LDS when
// P ints x 4 waves per block fit (up to ~138 cameras), else in the wave's own row of a device buffer (at most 2 GiB of rows:
// 4096 waves at 500 cameras).  MVBA_INDEX=global forces the device-memory histogram (the tests that the builds are identical).
// The temporaries live in `mem` from the counting pass to the end of the build, or to any early return.
struct DeviceIndexBuild {
  DevBufs mem;
  bool hist_lds = true;
  int idx_chunk = 32;  // points per wave
  long long idx_waves = 0;
  size_t idx_lds = 0;
  int *d_hist = nullptr;
  long long *d_cnt = nullptr;
};

int count_pairs_device(const IndexInput &in, const CreateKnobs &knobs, DeviceIndexBuild &dv, std::vector<long long> &cnt) {
  const long long N = in.N, P = in.P;
  dv.hist_lds = (size_t)P * sizeof(int) * IDX_WAVES <= 150 * 1024 && !knobs.index_global;
  const long long max_idx_waves = dv.hist_lds ? 4096 : std::max<long long>(IDX_WAVES, std::min<long long>(4096, (2LL << 30) / (4 * P)));
  dv.idx_chunk = (int)std::max<long long>(32, (N + max_idx_waves - 1) / max_idx_waves);
  dv.idx_waves = ((N + dv.idx_chunk - 1) / dv.idx_chunk + IDX_WAVES - 1) / IDX_WAVES * IDX_WAVES;
  dv.idx_lds = dv.hist_lds ? P * sizeof(int) * IDX_WAVES : 0;
  CR(dv.mem.alloc(&dv.d_hist, (size_t)dv.idx_waves * P));
  CR(dv.mem.alloc(&dv.d_cnt, (size_t)P));
  if (dv.hist_lds) {
    MVBA_HIP(hipFuncSetAttribute((const void *)k_idx_count<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dv.idx_lds));
    MVBA_HIP(hipFuncSetAttribute((const void *)k_idx_fill<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dv.idx_lds));
  } else {
    MVBA_HIP(hipMemsetAsync(dv.d_hist, 0, sizeof(int) * (size_t)dv.idx_waves * P, in.stream));
  }
  hipLaunchKernelGGL(dv.hist_lds ? k_idx_count<false> : k_idx_count<true>, dim3((unsigned)(dv.idx_waves / IDX_WAVES)), dim3(64 * IDX_WAVES), dv.idx_lds,
                     in.stream, N, in.m, (int)P, in.d_pt_ptr, in.d_cam, dv.idx_chunk, dv.d_hist, (const int *)nullptr);
  hipLaunchKernelGGL(k_idx_scan, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, in.stream, (int)P, (int)dv.idx_waves, dv.d_hist, dv.d_cnt);
  MVBA_HIP(hipMemcpyAsync(cnt.data(), dv.d_cnt, sizeof(long long) * P, hipMemcpyDeviceToHost, in.stream));
  MVBA_HIP(hipStreamSynchronize(in.stream));
  return MVBA_OK;
}

int build_index_device(const IndexInput &in, const SchurPlan &plan, DeviceIndexBuild &dv, DevBufs &engine, SchurIndex &ix, CreateTimer &timer) {
  const PairLists &L = plan.L;
  const PointRanges &R = plan.R;
  const long long N = in.N, P = in.P;
  const int m = in.m, nR = R.nR, VP = L.VP;
  hipStream_t stream = in.stream;
  DevBufs &tmp = dv.mem;
  int *d_pk = nullptr, *d_pl = nullptr, *d_pa = nullptr, *d_S = nullptr, *d_vp_ptr = nullptr;
  long long *d_vp_off = nullptr;
  CR(tmp.alloc(&d_pk, (size_t)L.T)); CR(tmp.alloc(&d_pl, (size_t)L.T)); CR(tmp.alloc(&d_pa, (size_t)L.T));
  CR(tmp.alloc(&d_S, (size_t)P)); CR(tmp.alloc(&d_vp_ptr, (size_t)P + 1)); CR(tmp.alloc(&d_vp_off, (size_t)VP + 1));
  MVBA_HIP(hipMemcpyAsync(d_S, L.S.data(), sizeof(int) * P, hipMemcpyHostToDevice, stream));
  MVBA_HIP(hipMemcpyAsync(d_vp_ptr, L.vp_ptr.data(), sizeof(int) * (P + 1), hipMemcpyHostToDevice, stream));
  MVBA_HIP(hipMemcpyAsync(d_vp_off, L.vp_off.data(), sizeof(long long) * (VP + 1), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(dv.hist_lds ? k_idx_fill<false> : k_idx_fill<true>, dim3((unsigned)(dv.idx_waves / IDX_WAVES)), dim3(64 * IDX_WAVES), dv.idx_lds,
                     stream, N, m, (int)P, in.d_pt_ptr, in.d_cam, dv.idx_chunk, dv.d_hist, d_S, d_vp_ptr, d_vp_off, d_pk, d_pl, d_pa,
                     (const int *)nullptr);
  MVBA_HIP(hipGetLastError());
  timer.lap("items sorted by pair");
  std::vector<long long> lo_tab((size_t)VP * (nR + 1));  // lower bounds of every list at every range boundary
  {
    long long *d_rl = nullptr, *d_lo = nullptr;
    CR(tmp.alloc(&d_rl, (size_t)nR + 1)); CR(tmp.alloc(&d_lo, lo_tab.size()));
    MVBA_HIP(hipMemcpyAsync(d_rl, R.lo.data(), sizeof(long long) * (nR + 1), hipMemcpyHostToDevice, stream));
    const long long nt = (long long)lo_tab.size();
    hipLaunchKernelGGL(k_idx_bounds, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, stream, VP, nR, d_vp_off, d_rl, d_pa, d_lo, (const int *)nullptr);
    MVBA_HIP(hipMemcpyAsync(lo_tab.data(), d_lo, sizeof(long long) * nt, hipMemcpyDeviceToHost, stream));
    MVBA_HIP(hipStreamSynchronize(stream));
    tmp.release(d_rl); tmp.release(d_lo);
  }
  std::vector<int> uid;
  number_units(in, plan, [&](int v, int r) { return lo_tab[(size_t)v * (nR + 1) + r]; }, ix, uid);
  timer.lap("units");
  if (plan.mode == SCHUR_SLOTS) {
    SlotWaves sw = make_slot_waves(in, plan, uid, ix);
    const long long n_waves = sw.n_waves;
    const int nSeg = sw.nSeg;
    CR(upload_range_o0(in, R, engine, ix));
    // device merge: the slots' list spans (from the units) go up, the step counts come back
    long long *d_slbeg = nullptr, *d_wbeg = nullptr;
    int *d_sllen = nullptr, *d_wsteps = nullptr;
    CR(tmp.alloc(&d_slbeg, sw.sl_beg.size())); CR(tmp.alloc(&d_sllen, sw.sl_len.size()));
    CR(tmp.alloc(&d_wsteps, (size_t)n_waves)); CR(tmp.alloc(&d_wbeg, (size_t)n_waves + 1));
    MVBA_HIP(hipMemcpyAsync(d_slbeg, sw.sl_beg.data(), sizeof(long long) * sw.sl_beg.size(), hipMemcpyHostToDevice, stream));
    MVBA_HIP(hipMemcpyAsync(d_sllen, sw.sl_len.data(), sizeof(int) * sw.sl_len.size(), hipMemcpyHostToDevice, stream));
    const int W = plan.W;
    const auto merge_count = W == LANES_W ? k_idx_merge<false, LANES_W> : k_idx_merge<false, PSTEP>;
    const auto merge_fill = W == LANES_W ? k_idx_merge<true, LANES_W> : k_idx_merge<true, PSTEP>;
    hipLaunchKernelGGL(merge_count, dim3((unsigned)n_waves), dim3(64), 0, stream, n_waves, nR, nSeg, slot_skew(W), SLOT_SEG, d_slbeg, d_sllen,
                       ix.d_range_o0, d_pk, d_pl, d_pa, d_wbeg, 0, (int)N, d_wsteps, (int *)nullptr, (int *)nullptr, (int *)nullptr,
                       (int *)nullptr, (const long long *)in.d_pt_ptr);
    std::vector<int> ws32(n_waves);
    MVBA_HIP(hipMemcpyAsync(ws32.data(), d_wsteps, sizeof(int) * n_waves, hipMemcpyDeviceToHost, stream));
    MVBA_HIP(hipStreamSynchronize(stream));  // (sl_beg / sl_len live until here)
    for (long long b = 0; b < n_waves; ++b) sw.w_steps[b] = ws32[b];
    timer.lap("slot merge (count)");
    long long total_steps = 0;
    CR(place_slot_steps(plan, sw, ix, total_steps));
    // the step-major arrays are written where the kernel will read them
    const size_t rows = (size_t)total_steps * W;
    CR(engine.alloc(&ix.d_it_k, rows)); CR(engine.alloc(&ix.d_it_l, rows)); CR(engine.alloc(&ix.d_it_a, rows));
    CR(engine.alloc(&ix.d_seg_end, ix.seg_end.size()));
    MVBA_HIP(hipMemcpyAsync(d_wbeg, sw.w_beg.data(), sizeof(long long) * (n_waves + 1), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(merge_fill, dim3((unsigned)n_waves), dim3(64), 0, stream, n_waves, nR, nSeg, slot_skew(W), SLOT_SEG, d_slbeg, d_sllen,
                       ix.d_range_o0, d_pk, d_pl, d_pa, d_wbeg, 0, (int)N, d_wsteps, ix.d_it_k, ix.d_it_l, ix.d_it_a, ix.d_seg_end, (const long long *)in.d_pt_ptr);
    MVBA_HIP(hipGetLastError());
    MVBA_HIP(hipStreamSynchronize(stream));
    timer.lap("slot merge (fill)");
    finish_slot_waves(plan, sw, total_steps, ix);
  } else {
    build_work_queues(in, plan, uid, ix);
    // the pair-major arrays stay where the fill kernel wrote them
    engine.adopt(tmp, d_pk); engine.adopt(tmp, d_pl); engine.adopt(tmp, d_pa);
    ix.d_it_k = d_pk; ix.d_it_l = d_pl; ix.d_it_a = d_pa;
  }
  tmp.release_all();
  ix.on_device = true;
  return MVBA_OK;
}

// ---------------------------------------------------------------- the engine's buffers, uploads, kernel attributes
int alloc_engine_buffers(mvba_handle *h, K1Tiles &t) {
  const long long N = h->N, nobs = h->nobs;
  const int m = h->m;
  h->cost_grid = (int)std::max<long long>(1, std::min<long long>(2048, (nobs + 255) / 256));
  h->n_partials = std::max(h->cost_grid, 4096);  // k_cost uses cost_grid blocks
  CR(h->mem.alloc(&h->d_obs_pt, nobs));
  CR(h->mem.alloc(&h->d_xy, nobs));
  h->n_tiles = (int)t.tiles.size() - 1;
  h->any_split = t.any_split;
  if (t.any_split) {
    t.tile_slot.resize(t.tiles.size(), -1);
    h->n_splits = (int)t.splits.size();
    CR(h->mem.alloc(&h->d_tile_slot, t.tile_slot.size()));
    CR(h->mem.alloc(&h->d_splits, t.splits.size()));
    CR(h->mem.alloc(&h->d_PLsplit, 9 * (size_t)t.n_split_slots));
    MVBA_HIP(hipMemcpy(h->d_tile_slot, t.tile_slot.data(), sizeof(int) * t.tile_slot.size(), hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(h->d_splits, t.splits.data(), sizeof(int4) * t.splits.size(), hipMemcpyHostToDevice));
  }
  CR(h->mem.alloc(&h->d_tiles, t.tiles.size()));
  for (int i = 0; i < 2; ++i) { CR(h->mem.alloc(&h->d_X[i], 3 * N)); CR(h->mem.alloc(&h->d_cam15[i], (size_t)CAM_IN * m)); }
  const int rec_slots = h->rec_compact ? REC_C : REC;
  CR(h->mem.alloc(&h->d_rec, (size_t)rec_slots * (nobs + 1)));  // + the all-zero record and point row the slot form's padding points at
  if (h->rec_compact) {  // the residuals beside the compact records, the padding record's among them
    CR(h->mem.alloc(&h->d_res, (size_t)nobs + 1));
    MVBA_HIP(hipMemset(h->d_res + nobs, 0, sizeof(double2)));
  }
  if (h->loss != LOSS_SQUARED) {
    CR(h->mem.alloc(&h->d_sqw, nobs + 1));
    MVBA_HIP(hipMemset(h->d_sqw, 0, sizeof(double) * (nobs + 1)));
  }
  CR(h->mem.alloc(&h->d_PL, 9 * N));
  CR(h->mem.alloc(&h->d_PB, (size_t)PBS * (N + 1)));
  MVBA_HIP(hipMemset(h->d_rec + (size_t)rec_slots * nobs, 0, sizeof(double2) * rec_slots));
  MVBA_HIP(hipMemset(h->d_PB + (size_t)PBS * N, 0, sizeof(double) * PBS));
  CR(h->mem.alloc(&h->d_Ab, h->n_Ab()));
  CR(h->mem.alloc(&h->d_Ared, (size_t)(h->D + 1) * h->ld));
  CR(h->mem.alloc(&h->d_Lblk, (size_t)((h->D + SBW - 1) / SBW) * SBW * SBW));
  CR(h->mem.alloc(&h->d_Ztiles, (size_t)((h->D + NB - 1) / NB) * NB * NB));
  CR(h->mem.alloc(&h->d_dxi, h->n9()));
  CR(h->mem.alloc(&h->d_dX, 3 * N));
  CR(h->mem.alloc(&h->d_partials, h->n_partials));
  CR(h->mem.alloc(&h->d_cost, 2));
  CR(h->mem.alloc(&h->d_flag, 1));
  CR(h->mem.alloc(&h->d_bar, 1 + 4 * (size_t)((9 * m + SBW - 1) / SBW)));  // progress words of the back-substitution
  MVBA_HIP(hipHostMalloc((void **)&h->h_cost, 4 * sizeof(double), hipHostMallocMapped));
  memset(h->h_cost, 0, 4 * sizeof(double));
  if (hipHostGetDevicePointer((void **)&h->d_mail, h->h_cost, 0) != hipSuccess) h->d_mail = nullptr;  // (no mapping: copy + sync as before)
  h->h_flag = reinterpret_cast<int *>(h->h_cost + 1);  // cost and flags come back in one copy
  return MVBA_OK;
}

// the pair-major index into the engine: what mvba_get_info reports, the device arrays of a device build, the rest uploaded
int upload_schur_index(mvba_handle *h, const SchurPlan &plan, SchurIndex &ix) {
  const int m = h->m;
  h->n_items = plan.L.T;
  h->n_items_offdiag = plan.L.T - plan.L.Tdiag;
  h->n_units = (int)ix.units.size();
  h->n_waves = ix.n_waves; h->slot_nR = ix.slot_nR; h->slot_nseg = ix.slot_nseg; h->n_slot_items = ix.n_slot_items;
  h->slot_w = ix.slot_w;
  h->index_on_device = ix.on_device;
  h->d_range_o0 = ix.d_range_o0;
  if (ix.on_device) { h->d_it_k = ix.d_it_k; h->d_it_l = ix.d_it_l; h->d_it_a = ix.d_it_a; h->d_seg_end = ix.d_seg_end; }
  const size_t P1 = (size_t)m * (m + 1) / 2 + 1;
  if (!ix.on_device) { CR(h->mem.alloc(&h->d_it_k, ix.it_k.size())); CR(h->mem.alloc(&h->d_it_l, ix.it_l.size())); CR(h->mem.alloc(&h->d_it_a, ix.it_a.size())); }
  CR(h->mem.alloc(&h->d_units, ix.units.size())); CR(h->mem.alloc(&h->d_unit_ptr, P1));
  CR(h->mem.alloc(&h->d_q_ptr, 9)); CR(h->mem.alloc(&h->d_q_units, ix.q_units.size()));
  CR(h->mem.alloc(&h->d_wdesc, ix.wdesc.size())); CR(h->mem.alloc(&h->d_wunits, ix.wunits.size()));
  if (!ix.on_device) CR(h->mem.alloc(&h->d_seg_end, ix.seg_end.size()));
  CR(h->mem.alloc(&h->d_prog, (size_t)h->slot_nR * std::max(1, h->slot_nseg) * PACE_STRIDE));
  if (!ix.seg_end.empty() && !ix.on_device) MVBA_HIP(hipMemcpy(h->d_seg_end, ix.seg_end.data(), sizeof(int) * ix.seg_end.size(), hipMemcpyHostToDevice));
  if (!ix.wdesc.empty()) {
    MVBA_HIP(hipMemcpy(h->d_wdesc, ix.wdesc.data(), sizeof(int4) * ix.wdesc.size(), hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(h->d_wunits, ix.wunits.data(), sizeof(int) * ix.wunits.size(), hipMemcpyHostToDevice));
  }
  CR(h->mem.alloc(&h->d_partial, (size_t)UNIT_STRIDE * ix.units.size()));
  if (!ix.it_k.empty()) {
    MVBA_HIP(hipMemcpy(h->d_it_k, ix.it_k.data(), sizeof(int) * ix.it_k.size(), hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(h->d_it_l, ix.it_l.data(), sizeof(int) * ix.it_l.size(), hipMemcpyHostToDevice));
    MVBA_HIP(hipMemcpy(h->d_it_a, ix.it_a.data(), sizeof(int) * ix.it_a.size(), hipMemcpyHostToDevice));
  }
  if (!ix.it_k.empty() || ix.on_device) {
    if (h->schur_mode == SCHUR_PAIRS) {
      std::vector<int4> qdesc(ix.units.size());  // descriptors in queue order (the kernel indexes both arrays by queue position)
      for (size_t i = 0; i < ix.q_units.size(); ++i) qdesc[i] = ix.units[ix.q_units[i]];
      MVBA_HIP(hipMemcpy(h->d_units, qdesc.data(), sizeof(int4) * qdesc.size(), hipMemcpyHostToDevice));
      int mx = 0;
      for (int x = 0; x < 8; ++x) mx = std::max(mx, ix.q_ptr[x + 1] - ix.q_ptr[x]);
      h->q_max = mx;
    }
    if (!ix.q_units.empty()) MVBA_HIP(hipMemcpy(h->d_q_units, ix.q_units.data(), sizeof(int) * ix.q_units.size(), hipMemcpyHostToDevice));
  }
  // the compact lane form: the descriptors in UNIT order -- a lane takes its pair's cameras (w = k << 16 | l) from its unit's
  if (h->rec_compact && !ix.units.empty()) MVBA_HIP(hipMemcpy(h->d_units, ix.units.data(), sizeof(int4) * ix.units.size(), hipMemcpyHostToDevice));
  if (h->schur_mode == SCHUR_SLOTS && h->n_slot_items) {  // the three step-major arrays -> one 256-byte (64 slots: 512, packed) row per step; they go
    const int W = h->slot_w, row = slot_idx_ints(W);
    const long long n_steps = h->n_slot_items / W;
    CR(h->mem.alloc(&h->d_it_x, (size_t)n_steps * row));
    hipLaunchKernelGGL(k_idx_interleave, dim3((unsigned)((n_steps * row + 255) / 256)), dim3(256), 0, h->stream, n_steps, W, row, h->d_it_k, h->d_it_l,
                       h->d_it_a, h->d_it_x);
    MVBA_HIP(hipGetLastError());
    MVBA_HIP(hipStreamSynchronize(h->stream));
    h->mem.release(h->d_it_k); h->mem.release(h->d_it_l); h->mem.release(h->d_it_a);
  }
  MVBA_HIP(hipMemcpy(h->d_unit_ptr, ix.unit_ptr.data(), sizeof(int) * P1, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemcpy(h->d_q_ptr, ix.q_ptr.data(), sizeof(int) * 9, hipMemcpyHostToDevice));
  MVBA_HIP(hipMemset(h->d_partial, 0, sizeof(double) * UNIT_STRIDE * std::max<size_t>(ix.units.size(), 1)));
  return MVBA_OK;
}

int upload_engine(mvba_handle *h, const mvba_problem *p, const std::vector<int> &obs_pt, const K1Tiles &t, const SchurPlan &plan, SchurIndex &ix) {
  const long long N = h->N, nobs = h->nobs;
  const int m = h->m;
  if (nobs) {
    MVBA_HIP(hipMemcpy(h->d_obs_pt, obs_pt.data(), sizeof(int) * nobs, hipMemcpyHostToDevice));
    if (p->xy_layout == 1) {  // image planes [m][N][2], as a caller's stack of per-image arrays lies in memory: into observation order here
      DevBufs tmp;
      double2 *planes = nullptr;  // (the host's strided gather of the same bytes: 0.1 s at 1 M points x 12 images)
      MVBA_HIP(hipMalloc((void **)&planes, sizeof(double2) * nobs));
      tmp.own(planes);
      hipError_t e = hipMemcpy(planes, p->xy, sizeof(double2) * nobs, hipMemcpyHostToDevice);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(k_xy_from_planes, dim3((unsigned)((N + 255) / 256), m), dim3(256), 0, 0, planes, N, m, h->d_xy);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
      }
      MVBA_HIP(e);
    } else {
      MVBA_HIP(hipMemcpy(h->d_xy, p->xy, sizeof(double2) * nobs, hipMemcpyHostToDevice));
    }
  }
  MVBA_HIP(hipMemcpy(h->d_tiles, t.tiles.data(), sizeof(int) * t.tiles.size(), hipMemcpyHostToDevice));
  // points without observations are never written by K1: their blocks stay zero (-> singular, ref :128)
  MVBA_HIP(hipMemset(h->d_PL, 0, sizeof(double) * 9 * std::max<long long>(N, 1)));
  MVBA_HIP(hipMemset(h->d_flag, 0, sizeof(int)));
  if (h->schur_mode == SCHUR_DENSE) {  // partial tiles of k_schur_dense: (tile pairs + one per camera) x 256 doubles per workgroup
    const int T = (9 * m + 15) / 16;
    int n_cu_dense = 256;
    hipDeviceGetAttribute(&n_cu_dense, hipDeviceAttributeMultiprocessorCount, h->device);
    h->dense_tiles = T * (T + 1) / 2 + m;
    h->dense_blocks = (int)std::max<long long>(1, std::min<long long>((N + dense_ch(T) - 1) / dense_ch(T), (long long)n_cu_dense * dense_wgs(T)));  // dense_wgs workgroups per CU (LDS and registers: see dense_ch)
    CR(h->mem.alloc(&h->d_dense_part, (size_t)h->dense_blocks * h->dense_tiles * 256));
    if (!plan.dense_obs.empty()) {
      CR(h->mem.alloc(&h->d_dense_obs, plan.dense_obs.size()));
      MVBA_HIP(hipMemcpy(h->d_dense_obs, plan.dense_obs.data(), sizeof(int) * plan.dense_obs.size(), hipMemcpyHostToDevice));
    }
  }
  if (h->use_pairs) CR(upload_schur_index(h, plan, ix));
  return MVBA_OK;
}

// opt in to large dynamic LDS: every kernel the engine can launch with more than the default, through the tables it launches from
int set_kernel_attributes(mvba_handle *h, const CreateKnobs &knobs) {
  const int m = h->m;
  const bool robust = h->loss != LOSS_SQUARED;
  auto set_lds = [](const void *f, size_t bytes) { return hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); };
  const size_t cam_lds = cam_lds_bytes(m, h->gcam, true);
  if (h->gcam) { CR(h->mem.alloc(&h->d_cam18, (size_t)m * CAM_LDS)); CR(h->mem.alloc(&h->d_dxi10, (size_t)m * DXI_LDS)); }
  for (int G : K5_LANES)  // every cell of K5's width rules (mvba_engine_host.h)
    for (int bt : TABLE_BLOCK_THREADS) {
      MVBA_HIP(set_lds(backsub_kernel(G, bt, false).fn(false), cam_lds));
      if (robust) MVBA_HIP(set_lds(backsub_kernel(G, bt, false).fn(true), cam_lds));
    }
  MVBA_HIP(set_lds((const void *)k_chol_super, SUPER_LDS));
  MVBA_HIP(set_lds((const void *)k_chol_backsolve_all<true>, BACKSOLVE_LDS));
  {
    // the persistent back-substitution needs its whole grid resident: at most one workgroup per CU
    int per_cu = 0;
    MVBA_HIP(hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, h->device));
    MVBA_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_chol_backsolve_all<true>, SUPER_THREADS, BACKSOLVE_LDS));
    h->chol_onepass = per_cu >= 1 && !knobs.chol_launches;
    h->trail64_min = knobs.trail64_min;
    h->barrier_polls = knobs.barrier_polls;
  }
  const size_t k1_lds = k1_lds_bytes(m, h->gcam, h->k1_threads);
  MVBA_HIP(set_lds(resid_jac_kernel(h->gcam, h->loss).fn(false), k1_lds));
  if (h->rec_compact) MVBA_HIP(set_lds((const void *)k_resid_jac<false, LOSS_SQUARED, CompactRec>, k1_lds));
  MVBA_HIP(set_lds(cost_kernel(false, h->loss).fn(false), cam_lds));
  MVBA_HIP(set_lds((const void *)k_residuals<false>, cam_lds));
  if (robust) {
    MVBA_HIP(set_lds(resid_jac_kernel(h->gcam, h->loss).fn(true), k1_lds));
    MVBA_HIP(set_lds(cost_kernel(false, h->loss).fn(true), cam_lds));
  }
  if (h->schur_mode == SCHUR_DENSE) {  // the limit of the INSTANTIATION -- its largest camera count -- so that engines with other m share it
    const int T = (9 * m + 15) / 16;
    MVBA_HIP(set_lds(dense_kernel(T, h->d_dense_obs != nullptr).fn(robust), dense_lds_bytes(T, 16 * T / 9)));
  }
  return MVBA_OK;
}

// ---------------------------------------------------------------- mvba_create
int build_engine(mvba_handle *h, const mvba_problem *p, const CreateKnobs &knobs, const std::vector<int> &obs_pt, K1Tiles &tiles, CreateTimer &timer) {
  const long long N = h->N, nobs = h->nobs;
  const int m = h->m;
  if (p->device >= 0) MVBA_HIP(hipSetDevice(p->device));
  MVBA_HIP(hipGetDevice(&h->device));
  // the topology goes up first: the Schur index is built from it on the device
  MVBA_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  CR(h->mem.alloc(&h->d_pt_ptr, N + 1));
  CR(h->mem.alloc(&h->d_cam, nobs));
  MVBA_HIP(hipMemcpy(h->d_pt_ptr, p->pt_ptr, sizeof(long long) * (N + 1), hipMemcpyHostToDevice));
  if (nobs) MVBA_HIP(hipMemcpy(h->d_cam, p->cam_idx, sizeof(int) * nobs, hipMemcpyHostToDevice));
  timer.lap("device, topology upload");
  h->k1_threads = k1_block_threads(m, h->gcam);

  // The index is built on the DEVICE (k_idx_*) unless MVBA_INDEX=host keeps the host threads
  const bool dev_build = N > 0 && nobs > 0 && !knobs.index_host;
  const IndexInput in{p, N, nobs, (long long)m * (m + 1) / 2, m,
                      (int)std::max(1u, std::min({std::thread::hardware_concurrency(), 16u, (unsigned)m})), h->stream, h->d_pt_ptr, h->d_cam};
  DeviceIndexBuild dv;  // (its temporaries go with this scope)
  SchurPlan plan;
  SchurIndex ix;
  // The record layout is the engine's: compact exactly where K3 takes the lane form -- the one form with arithmetic to
  // spare for the omega rows --, the loss is squared and K1 holds the camera table in LDS; MVBA_REC=full keeps the 128-byte record
  const bool compact_rec = h->loss == LOSS_SQUARED && !h->gcam && !knobs.rec_full;
  CR(decide_schur_form(in, knobs, h->loss, compact_rec, h->device, [&](std::vector<long long> &cnt) {
    return dev_build ? count_pairs_device(in, knobs, dv, cnt) : count_pairs_host(in, cnt);
  }, plan, timer));
  h->schur_mode = plan.mode;
  h->use_pairs = plan.mode != SCHUR_DENSE;
  h->rec_compact = plan.mode == SCHUR_SLOTS && plan.W == LANES_W && compact_rec;
  h->lane_places = plan.mode == SCHUR_SLOTS && plan.W == LANES_W ? plan.lane_places : 0;
  if (h->use_pairs) CR(dev_build ? build_index_device(in, plan, dv, h->mem, ix, timer) : build_index_host(in, plan, h->mem, ix, timer));
  timer.lap("queues / wave descriptors");

  CR(alloc_engine_buffers(h, tiles));
  timer.lap("allocations");
  CR(upload_engine(h, p, obs_pt, tiles, plan, ix));
  timer.lap("uploads");
  CR(set_kernel_attributes(h, knobs));
  timer.lap("attributes");
  return MVBA_OK;
}

int create_engine(const mvba_problem *p, int loss, double loss_b, mvba_handle **out) {
  if (!p || !out) return fail(MVBA_ERR_BADARG, "null argument");
  const CreateKnobs knobs = read_create_knobs();
  CreateTimer timer{knobs.timing};
  std::vector<int> obs_pt;
  CR(validate_problem(p, obs_pt));
  timer.lap("validate, obs_pt");
  K1Tiles tiles = build_k1_tiles(p);
  timer.lap("K1 tiles");

  mvba_handle *h = new mvba_handle();
  const int m = p->n_images;
  h->N = p->n_points; h->nobs = p->n_obs; h->m = m; h->gauge_axis = p->gauge_axis; h->f0 = p->f0; h->D = 9 * m - 7; h->ld = (h->D + 3) & ~3;
  h->loss = loss; h->loss_b = loss_b;
  h->gcam = m > LDS_CAMERAS;
  h->force_big = knobs.force_big;
  h->check_solve = knobs.check_solve;
  h->check_solve_tol = knobs.check_solve_tol;
  if (int rc = build_engine(h, p, knobs, obs_pt, tiles, timer)) {  // every failure past this point: the half-built engine goes, once
    const std::string err = g_err;  // (mvba_destroy synchronises the stream: keep the first error's text)
    mvba_destroy(h);
    g_err = err;
    return rc;
  }
  *out = h;
  return MVBA_OK;
}

#undef CR
