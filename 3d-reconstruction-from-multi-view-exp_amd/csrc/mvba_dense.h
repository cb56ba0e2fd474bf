// K3, the dense form (every point seen by every camera, up to 21 cameras) -- kernels, gfx950: k_schur_dense on the f64 matrix
// cores and k_schur_dense_finish, which sums the workgroups' partial tiles into the packed strips.
//
// Included by mvba.hip inside its device-code namespace, after mvba_schur.h: uses REC, PBS and strip_offset of mvba_device.h (its
// robust form takes a LossArgs).  mvba_d4 is defined here and used by mvba_solve.h.  The host side (dense_kernel, dense_lds_bytes, launch_schur)
// is in mvba.hip.

// ------------------------------------------------------------------ K3 (dense visibility: every point seen by every camera)
// The reference's own scenes (euclidiean_reconstruction.py, affine_reconstruction.py, BASELINE config 2) and the pipeline test at
// 1 M points x 12 images have FULL visibility and a dozen or two cameras.  The pair-major forms above then walk m (m + 1) / 2 items
// per point through gathers and an index of their own (78 items and 0.9 GB of index per million points at 12 cameras: 4.9 ms per
// solve, 63 ps per item against 30 at config 3) although a point's m records are ONE contiguous range and every pair is present.
// With E_a^-1 = R_a R_a^T (3 x 3 Cholesky) and the scaled camera Jacobian J~_ak (2 x 9: f | u, v (1 / f0) | t (-J_X) | omega)
//   G_a = [R_a^T J_Xak^T J~_ak]_k   (3 x 9m),        A = blockdiag(2 H_k + c diag(2 H_k)) - 4 sum_a G_a^T G_a,
//   H_k = sum_a J~_ak^T J~_ak,                        b_k = 2 sum_a J~_ak^T (J_Xak E_a^-1 dP_a - e_ak)
// -- one symmetric rank-3N update of a 9m x 9m matrix: a GEMM, on the f64 matrix cores, over records streamed ONCE.
// A workgroup takes a chunk of points (dense_ch: 4 or 8) at a time: their records and point rows go into LDS with contiguous 16-byte loads; a thread per
// observation forms J_X R and the right-hand-side vector w; the rows of G are written to LDS once (each is read by up to T tile
// pairs); wave w then owns the 16 x 16 tile pairs w, w + 4, ... of the upper triangle (four consecutive rows of G -- of whichever
// points -- are one v_mfma_f64_16x16x4: no padding of K) and the per-camera tiles [J~ | w]^T [J~ | w] (two points per MFMA) of the
// cameras w, w + 4, ...  Partial tiles per workgroup, summed in workgroup order by k_schur_dense_finish: no atomics, bitwise
// reproducible.  No index at all: mvba_create skips the pair-major index for such scenes.
typedef double mvba_d4 __attribute__((ext_vector_type(4)));
// Points per chunk (= producer waves) and workgroups per CU.  Up to 7 tiles (12 cameras) the kernel needs at most 126 registers: four
// waves fit a SIMD, so TWO 8-wave workgroups of 4-point chunks (~53 KB of LDS each) share a CU and fill each other's barrier waits
// (1.335 -> 1.260 ms at 1 M x 12, 1.48 -> 1.32 at 2 M x 6; three workgroups: worse again).  8 tiles take 154 registers -- three waves
// per SIMD -- and stay with one 12-wave workgroup of 8-point chunks (two of the small ones cannot both be resident: 1.65 -> 1.82 ms
// at 14 cameras); beyond that eight consumer + four producer waves.  (tools/dense_ch.sh, profiles/r05_dense_form.txt)
constexpr int dense_ch(int T) { return T == 8 ? 8 : 4; }
constexpr int dense_wgs(int T) { return T <= 7 ? 2 : 1; }
constexpr int DENSE_MAX_TILES = 12;  // 9 m <= 192: m <= 21 cameras (78 tile pairs: 20 accumulators of 4 doubles per lane)
__device__ __forceinline__ int dense_tile_elem(int row, int col) { return ((row >> 2) << 6) | ((row & 3) << 4) | col; }  // C/D layout: col = l & 15, row = (l >> 4) + 4 reg

constexpr int dense_pair_ti(int p, int T) { int a = 0; while (p >= T - a) { p -= T - a; ++a; } return a; }
constexpr int dense_pair_tj(int p, int T) { int a = 0; while (p >= T - a) { p -= T - a; ++a; } return a + p; }
constexpr int dense_consumers(int T) { return T <= 8 ? 4 : 8; }  // consumer waves: at most ~10 tile pairs (40 accumulator doubles) each
constexpr bool dense_tile_used(int u, int T, int wave) {  // does consumer wave `wave` own a pair with tile u?
  const int P = T * (T + 1) / 2, NC = dense_consumers(T);
  for (int p = wave; p < P; p += NC)
    if (dense_pair_ti(p, T) == u || dense_pair_tj(p, T) == u) return true;
  // (its spare slots repeat the last pair)
  return (P + NC - 1) / NC * NC - NC + wave >= P && (dense_pair_ti(P - 1, T) == u || dense_pair_tj(P - 1, T) == u);
}
// the main products of one chunk for consumer wave WAVE: its tile pairs p = NC q + WAVE are known at compile time, so the operand of a
// tile is read from LDS ONCE per four rows of G and used from its register by every pair that needs it (two reads per MFMA, with
// the tiles indexed at run time, kept the LDS half busy under the matrix cores).  (The pair -> tile arithmetic goes through class
// templates: called as constexpr FUNCTIONS inside the unrolled loops it was evaluated at run time, with the registers indexed
// through s_set_gpr_idx.)
template <int T, int WAVE, int Q>
struct DensePair {
  static constexpr int P = T * (T + 1) / 2, NC = dense_consumers(T);
  static constexpr int p = NC * Q + WAVE < P ? NC * Q + WAVE : P - 1;  // (a spare slot repeats the last pair: computed, never stored)
  static constexpr int ti = dense_pair_ti(p, T), tj = dense_pair_tj(p, T);
};
template <int T, int WAVE, int U>
struct DenseUsed { static constexpr bool v = dense_tile_used(U, T, WAVE); };
template <int T, int WAVE, int... U>
__device__ __forceinline__ void dense_load_tiles(const double *row, double (&t)[T], std::integer_sequence<int, U...>) {
  ((t[U] = DenseUsed<T, WAVE, U>::v ? row[16 * U] : 0.0), ...);
}
template <int T, int WAVE, int... Q>
__device__ __forceinline__ void dense_mfma_pairs(const double (&ts)[T], const double (&t)[T], mvba_d4 *acc, std::integer_sequence<int, Q...>) {
  ((acc[Q] = __builtin_amdgcn_mfma_f64_16x16x4f64(ts[DensePair<T, WAVE, Q>::ti], t[DensePair<T, WAVE, Q>::tj], acc[Q], 0, 0, 0)), ...);
}
template <int T, int WAVE, int CH>
__device__ __forceinline__ void dense_main_mfma(const double *sG, const double *sSgn, int li, int lk, mvba_d4 *acc) {
  constexpr int P = T * (T + 1) / 2, NC = dense_consumers(T), NPW = (P + NC - 1) / NC, W = 16 * T;
#pragma unroll
  for (int g = 0; g < 3 * CH / 4; ++g) {  // four rows of G per MFMA: sum_r s_r g_r^T g_r (s = +-1: E^-1 = R S R^T), the sign on the left operand
    double t[T], ts[T];
    dense_load_tiles<T, WAVE>(sG + (size_t)(4 * g + lk) * W + li, t, std::make_integer_sequence<int, T>{});
    const double sg = sSgn[4 * g + lk];
#pragma unroll
    for (int u = 0; u < T; ++u) ts[u] = t[u] * sg;
    dense_mfma_pairs<T, WAVE>(ts, t, acc, std::make_integer_sequence<int, NPW>{});
  }
}

// Two roles in a workgroup, one barrier per chunk: waves 0-3 multiply chunk i (main pairs and camera tiles out of the buffers of
// parity i & 1) while the producer waves -- one per point of a chunk -- build chunk i + 1 into the other buffers, each taking its
// point from its records (fetched into registers a chunk earlier) to the rows of G on its own, so the producers need no barrier
// among themselves.  (With every wave doing every phase in turn -- four barriers per chunk -- the workgroups of a CU ran in
// lockstep and the phases never overlapped: 1.55 ms at 1 M x 12 for 0.81 ms of MFMA phase; with four producer waves of two points
// each the producers were the longer role: 1.90 ms.)
// ROBUST: the records are scaled by sqrt(w) (K1); the constant columns of an observation become sqrt(w) / f0
// instead of 1 / f0 -- the per-(point, camera) factor sF takes sqrt(w) from `sqw`, fetched with the records.
#define MVBA_DENSE_ARGS                                                                                                   \
  const double2 *__restrict__ rec, const double *__restrict__ PB, const int *__restrict__ obs_of, long long N, int m, double cu, \
      double *__restrict__ part
template <int T, bool TABLE, bool ROBUST = false, typename... Robust>  // TABLE: the records of a point through obs_of (missing observations), otherwise one contiguous range
__global__ __launch_bounds__(64 * (dense_consumers(T) + dense_ch(T))) void k_schur_dense(MVBA_DENSE_ARGS, Robust... robust) {
  constexpr int NC = dense_consumers(T);           // consumer waves (4 + 8 producers up to 8 tiles, 8 + 4 beyond)
  constexpr int P = T * (T + 1) / 2, NPW = (P + NC - 1) / NC, W = 16 * T, NCW = ((16 * T) / 9 + NC - 1) / NC;
  constexpr int CH = dense_ch(T);       // points per chunk = producer waves (the double-buffered rows must fit the LDS beside each other)
  constexpr int MMAX = (16 * T) / 9;               // cameras at most
  constexpr int NTHR = 64 * (NC + CH);
  extern __shared__ double2 dsm[];
  double *sG = reinterpret_cast<double *>(dsm);                     // [2][3 CH][W]
  double *sB = sG + (size_t)2 * 3 * CH * W;                         // [2][CH m][2][16]: rows x, y of [J~ (9) | w | 0 ...]
  double2 *sScr = reinterpret_cast<double2 *>(sB + (size_t)2 * CH * m * 32);  // per producer wave: records [m][8], point row [8]
  double *sFlag = reinterpret_cast<double *>(sScr + (size_t)CH * (m * REC + 8));  // per producer wave: [m] 1 for an observation, 0 for a missing one
  double *sSgn = sFlag + (size_t)CH * m;                            // [2][3 CH]: the signs of the rows of G
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;  // (wave through readfirstlane -- scalar address arithmetic for the producers -- made every shape slower: 1.36 -> 1.55 ms at 1 M x 12, 2.95 -> 12.6 at 20 cameras)
  const long long n_chunks = (N + CH - 1) / CH;
  // what no phase ever writes stays zero: the columns of G beyond 9 m, the columns 10..15 of the camera rows
  for (int e = threadIdx.x; e < 2 * 3 * CH * W; e += NTHR) sG[e] = 0.0;
  for (int e = threadIdx.x; e < 2 * CH * m * 32; e += NTHR) sB[e] = 0.0;
  __syncthreads();
  if (wave >= NC) {
    // ---------------- producer: point pw of every chunk of this workgroup.  (Without the staging -- a lane per (camera, column)
    // fetching its four record slots itself -- the per-lane loads cost more than the staging saves: 1.82 against 1.40 ms.)
    const int pw = wave - NC;
    // The producers are the longer role (role trace, profiles/r05_dense_form.txt: 5,350 cycles of work per chunk against the consumers' 4,480 + 1,400 at
    // the barrier, 1 M x 12) and, as the later-dispatched waves of their SIMD, the losers of its issue arbitration (older first at
    // equal priority): they ask for the higher priority once, here.
    __builtin_amdgcn_s_setprio(1);
    double2 *sR = sScr + (size_t)pw * (m * REC + 8), *sP = sR + (size_t)m * REC;
    constexpr int NPRE = (MMAX * REC + 63) / 64, NIT = (MMAX * 10 + 63) / 64;
    // TWO chunks' records in flight per wave (sets A and B, used in turn): with one, a CU had 8 waves x 1.5 KB outstanding against
    // ~2 us of loaded memory latency -- 1.5 TB/s over the chip, which is where the kernel sat at every camera count (~1.0 ms per
    // million points x 12 cameras whatever the matrix cores had to do)
    double2 preA[NPRE], prepbA, preB[NPRE], prepbB;
    double swA[NPRE], swB[NPRE];                   // ROBUST: sqrt(w) of the observation of every record slot a lane fetched
    bool lvA, lvB;
    int oidA[NPRE], oidB[NPRE], oid_next[NPRE];    // (obs_of != nullptr) the observations of a set's point / of the point fetched next
    double *sF = sFlag + (size_t)pw * m;
    auto fetch_ids = [&](long long ch) {           // the table row of chunk ch's point (one entry per record: eight lanes share it)
      const long long a = ch * CH + pw;
#pragma unroll
      for (int u = 0; u < NPRE; ++u) {
        const int e = lane + 64 * u;
        const int got = obs_of[(size_t)min(a, N - 1) * m + min(e >> 3, m - 1)], msk = (a < N && e < m * REC) ? -1 : 0;
        oid_next[u] = (got & msk) | ~msk;          // (-1 outside; the load itself is unconditional, see fetch)
      }
    };
    auto fetch = [&](long long ch, double2 (&pre)[NPRE], int (&oid)[NPRE], double2 &prepb, bool &lv, double (&sw)[NPRE]) {  // this wave's records and point row of chunk ch (zeros past the last point)
      // The loads are UNCONDITIONAL on clamped addresses and what must be zero (a missing observation, a point past the end) is
      // zeroed on the bit pattern in build(): behind a lane-dependent branch the compiler cannot count the loads in flight and
      // waits for all of them (vmcnt(0)) -- the other set's too, which is the one meant to stay in flight
      const long long a = ch * CH + pw;
      const bool live = lv = a < N;
      if (TABLE) {                                 // through the table read a chunk earlier
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
          oid[u] = oid_next[u];
          pre[u] = rec[(size_t)max(oid[u], 0) * REC + ((lane + 64 * u) & 7)];
          if constexpr (ROBUST) sw[u] = (robust, ...).sqw[max(oid[u], 0)];
        }
      } else {
        const double2 *src = rec + (size_t)min(a, N - 1) * m * REC;
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
          pre[u] = src[min(lane + 64 * u, m * REC - 1)];
          oid[u] = live ? 0 : -1;
          if constexpr (ROBUST) sw[u] = (robust, ...).sqw[(size_t)min(a, N - 1) * m + min((lane + 64 * u) >> 3, m - 1)];
        }
      }
      prepb = reinterpret_cast<const double2 *>(PB + (size_t)min(a, N - 1) * PBS)[lane & 7];
    };
    auto keep = [](bool c, double2 v) -> double2 {  // c ? v : 0 without a branch the load could sink under
      const long long msk = c ? -1LL : 0LL;
      return double2{__longlong_as_double(__double_as_longlong(v.x) & msk), __longlong_as_double(__double_as_longlong(v.y) & msk)};
    };
    auto build = [&](int buf, const double2 (&pre)[NPRE], const int (&oid)[NPRE], const double2 &prepb, bool lv, const double (&sw)[NPRE]) {  // registers -> the rows of G and the camera rows of this wave's point in buffer `buf`
#pragma unroll
      for (int u = 0; u < NPRE; ++u) {
        const int e = lane + 64 * u;
        if (e < m * REC) sR[e] = keep(oid[u] >= 0, pre[u]);
        if (e < m * REC && (e & 7) == 0) sF[e >> 3] = oid[u] >= 0 ? (ROBUST ? sw[u] : 1.0) : 0.0;
      }
      sP[lane & 7] = keep(lv, prepb);             // (every lane, eight copies of each slot: a store under `lane < 8` drew a vmcnt(0))
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      // point row: E^-1 (6) | E^-1 dP (3) | sign code | R lower triangular (r00 r10 r20 r11 r21 r22) of E^-1 = R S R^T (k_point_inv), the same for every lane
      const double *pb = reinterpret_cast<const double *>(sP);
      const double d0 = pb[6], d1 = pb[7], d2 = pb[8];
      const double r00 = pb[10], r10 = pb[11], r20 = pb[12], r11 = pb[13], r21 = pb[14], r22 = pb[15];
      double *gB = sB + ((size_t)buf * CH + pw) * m * 32;
      double *gG = sG + ((size_t)buf * 3 * CH + (size_t)3 * pw) * W;
      if (lane < 3) sSgn[(size_t)buf * 3 * CH + 3 * pw + lane] = (((int)pb[9] - 1) >> lane) & 1 ? -1.0 : 1.0;
      // a lane per (camera k, column j <= 9): column j of J~ (f | u, v (1 / f0) | t (-J_X) | omega) into the two camera rows and
      // G[r][9 k + j] = (J_X R)[:, r] . J~[:, j] (E^-1 = R R^T); j = 9: w = J_X E^-1 dP - e, the tenth column of the camera rows
#pragma unroll
      for (int u = 0; u < NIT; ++u) {
        const int e = lane + 64 * u, k = e / 10, j = e - 10 * k;
        if (e < 10 * m) {
          const double2 *r = sR + (size_t)k * REC;
          const double2 x0 = r[0], x1 = r[1], x2 = r[2];
          const double2 cv = r[j == 0 ? 3 : (j < 6 ? (j < 3 ? 0 : j - 3) : (j < 9 ? j - 2 : 7))];
          if (j == 9) {
            gB[(size_t)k * 32 + 9] = x0.x * d0 + x1.x * d1 + x2.x * d2 - cv.x;
            gB[(size_t)k * 32 + 25] = x0.y * d0 + x1.y * d1 + x2.y * d2 - cv.y;
          } else {
            const double sg = (j >= 3 && j < 6) ? -1.0 : 1.0, live = sF[k] * cu;  // (the constant columns 1 / f0 of an observation that exists)
            const double jx = j == 1 ? live : (j == 2 ? 0.0 : sg * cv.x), jy = j == 2 ? live : (j == 1 ? 0.0 : sg * cv.y);
            gB[(size_t)k * 32 + j] = jx;
            gB[(size_t)k * 32 + 16 + j] = jy;
            double *g = gG + 9 * k + j;
            g[0] = (x0.x * r00 + x1.x * r10 + x2.x * r20) * jx + (x0.y * r00 + x1.y * r10 + x2.y * r20) * jy;
            g[W] = (x1.x * r11 + x2.x * r21) * jx + (x1.y * r11 + x2.y * r21) * jy;
            g[2 * W] = (x2.x * r22) * jx + (x2.y * r22) * jy;
          }
        }
      }
    };
    long long ch = blockIdx.x;
    const long long gs = gridDim.x;
    // (a fetch past the last chunk loads nothing: zero records nobody reads; fetch_ids likewise -1)
    if (TABLE) fetch_ids(ch);
    fetch(ch, preA, oidA, prepbA, lvA, swA);
    if (TABLE) fetch_ids(ch + gs);
    fetch(ch + gs, preB, oidB, prepbB, lvB, swB);
    if (TABLE) fetch_ids(ch + 2 * gs);
    build(0, preA, oidA, prepbA, lvA, swA);
    fetch(ch + 2 * gs, preA, oidA, prepbA, lvA, swA);
    if (TABLE) fetch_ids(ch + 3 * gs);
    __syncthreads();
    // One barrier per chunk, as the consumers; the sets alternate: B holds chunk ch + 1, A chunk ch + 2.  Nothing in the body is
    // conditional (behind `if (ch + gs < n_chunks)` the compiler lost count of the loads in flight and waited vmcnt(0) for both
    // sets): past the last chunk a build writes a chunk of zeros into the buffer nobody reads any more.
    for (int b = 0; ch < n_chunks;) {
      build(b ^ 1, preB, oidB, prepbB, lvB, swB);
      fetch(ch + 3 * gs, preB, oidB, prepbB, lvB, swB);
      if (TABLE) fetch_ids(ch + 4 * gs);
      __syncthreads();
      ch += gs, b ^= 1;
      if (ch >= n_chunks) break;
      build(b ^ 1, preA, oidA, prepbA, lvA, swA);
      fetch(ch + 3 * gs, preA, oidA, prepbA, lvA, swA);
      if (TABLE) fetch_ids(ch + 4 * gs);
      __syncthreads();
      ch += gs, b ^= 1;
    }
    return;
  }
  // ---------------- consumer: tile pairs NC q + wave of the upper triangle (row-major), cameras NC q + wave
  mvba_d4 acc[NPW], cacc[NCW];
#pragma unroll
  for (int q = 0; q < NPW; ++q) acc[q] = mvba_d4{0, 0, 0, 0};
#pragma unroll
  for (int q = 0; q < NCW; ++q) cacc[q] = mvba_d4{0, 0, 0, 0};
  __syncthreads();  // chunk 0 is built
  int b = 0;
  for (long long ch = blockIdx.x; ch < n_chunks; ch += gridDim.x, b ^= 1) {
    const double *bG = sG + (size_t)b * 3 * CH * W, *bB = sB + (size_t)b * CH * m * 32, *bS = sSgn + (size_t)b * 3 * CH;
    switch (wave) {  // (uniform)
      case 0: dense_main_mfma<T, 0, CH>(bG, bS, li, lk, acc); break;
      case 1: dense_main_mfma<T, 1, CH>(bG, bS, li, lk, acc); break;
      case 2: dense_main_mfma<T, 2, CH>(bG, bS, li, lk, acc); break;
      case 3: dense_main_mfma<T, 3, CH>(bG, bS, li, lk, acc); break;
      case 4: dense_main_mfma<T, 4 % NC, CH>(bG, bS, li, lk, acc); break;  // (cases 4..7 exist with eight consumers only)
      case 5: dense_main_mfma<T, 5 % NC, CH>(bG, bS, li, lk, acc); break;
      case 6: dense_main_mfma<T, 6 % NC, CH>(bG, bS, li, lk, acc); break;
      default: dense_main_mfma<T, 7 % NC, CH>(bG, bS, li, lk, acc); break;
    }
#pragma unroll
    for (int g = 0; g < CH / 2; ++g) {  // the per-camera tiles: rows (point 2 g, x), (2 g, y), (2 g + 1, x), (2 g + 1, y)
      const int pa = 2 * g + (lk >> 1), d = lk & 1;
#pragma unroll
      for (int q = 0; q < NCW; ++q) {
        const int k = min(NC * q + wave, m - 1);
        const double v = bB[(size_t)(pa * m + k) * 32 + 16 * d + li];
        cacc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, cacc[q], 0, 0, 0);
      }
    }
    __syncthreads();  // this chunk's buffers may be rebuilt, the next chunk's are complete
  }
  double *out = part + (size_t)blockIdx.x * (P + m) * 256;
#pragma unroll
  for (int q = 0; q < NPW; ++q) {
    const int p = NC * q + wave;
    if (p < P)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(size_t)p * 256 + r * 64 + lane] = acc[q][r];
  }
#pragma unroll
  for (int q = 0; q < NCW; ++q) {
    const int k = NC * q + wave;
    if (k < m)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(size_t)(P + k) * 256 + r * 64 + lane] = cacc[q][r];
  }
}

// One wave per element of the packed strips [A | b]: the workgroups' partial tiles summed in workgroup order (lane l takes the
// workgroups l, l + 64, ... in order, then a fixed tree).
__global__ __launch_bounds__(256) void k_schur_dense_finish(int m, int T, int blocks, const double *__restrict__ part, double c,
                                                            double *__restrict__ Afull, double *__restrict__ bfull) {
  const long long e = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, P = T * (T + 1) / 2;
  const long long nA = (long long)strip_offset(m, m);
  if (e >= nA + 9 * m) return;
  const size_t bstride = (size_t)(P + m) * 256;
  auto total = [&](int tile, int elem) {
    double t = 0.0;
    for (int b = lane; b < blocks; b += 64) t += part[(size_t)b * bstride + (size_t)tile * 256 + elem];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
    return t;  // (valid in lane 0)
  };
  if (e < nA) {
    int k = 0;
    while (k + 1 < m && (long long)strip_offset(k + 1, m) <= e) ++k;
    const int Wk = 9 * (m - k), rem = (int)(e - (long long)strip_offset(k, m)), i = rem / Wk, cr = rem - i * Wk, l = k + cr / 9, j = cr - 9 * (l - k);
    const int gi = 9 * k + i, gj = 9 * l + j, lo = min(gi, gj), hi = max(gi, gj), ti = lo >> 4, tj = hi >> 4;
    double v = -4.0 * total(ti * T - ti * (ti - 1) / 2 + (tj - ti), dense_tile_elem(lo & 15, hi & 15));
    if (k == l) {
      const double hk = total(P + k, dense_tile_elem(i, j));
      v += 2.0 * hk * (i == j ? 1.0 + c : 1.0);  // G_k and its Marquardt term c diag(G_k)   (ref :123-125)
    }
    if (lane == 0) Afull[e] = v;
  } else {
    const int q = (int)(e - nA), k = q / 9, j = q - 9 * k;
    const double v = 2.0 * total(P + k, dense_tile_elem(j, 9));  // 2 Jc_k^T (Jx_k E^-1 dP - e)
    if (lane == 0) bfull[q] = v;
  }
}
