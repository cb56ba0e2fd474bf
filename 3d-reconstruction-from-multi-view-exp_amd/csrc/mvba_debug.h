// The engine's diagnostics on the host: the snapshot log (mvba_snapshot*), mvba_set_profiling, mvba_get_stats, mvba_reset_stats,
// mvba_get_info and mvba_debug_read.  debug_buffer() is the one place that knows a buffer id of mvba_debug_read: it answers the
// count and the filler together, so a new id is one case there.
//
// Included by mvba.hip after mvba_cov_host.h: uses mvba_engine.h (mvba_handle, read_state, write_state, sync_and_drain) and the
// expansions of mvba_engine_host.h (expand_compact_record, record_to_*, expand_packed_A).
#include <functional>

extern "C" {

// ---- debug log: per-iteration copies of the committed state, device-resident (ref :89-98, :175-183, :204-206)
namespace {
constexpr int SNAP_SLAB = 8;  // log entries per device allocation
size_t snap_stride(const mvba_handle *h) { return (3 * (size_t)h->N + (size_t)CAM_IN * h->m + 1) & ~(size_t)1; }
// log entry i: points [3 N], then cameras [m][CAM_IN] (its slab must exist)
double *snap_entry(const mvba_handle *h, long long i) { return h->snap_slabs[(size_t)(i / SNAP_SLAB)] + snap_stride(h) * (size_t)(i % SNAP_SLAB); }
}  // namespace

int mvba_snapshot(mvba_handle *h) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  if (!h->have_params) return fail(MVBA_ERR_STATE, "no parameters set");
  MVBA_HIP(hipSetDevice(h->device));
  if ((size_t)(h->n_snap / SNAP_SLAB) >= h->snap_slabs.size()) {
    double *p = nullptr;
    int rc = h->mem.alloc(&p, snap_stride(h) * SNAP_SLAB);
    if (rc) return rc;
    h->snap_slabs.push_back(p);
  }
  double *dst = snap_entry(h, h->n_snap);
  // same stream as the kernels: ordered after everything that wrote the committed state and before whatever
  // overwrites it; the host does not wait
  MVBA_HIP(hipMemcpyAsync(dst, h->d_X[h->cur], sizeof(double) * 3 * h->N, hipMemcpyDeviceToDevice, h->stream));
  MVBA_HIP(hipMemcpyAsync(dst + 3 * h->N, h->d_cam15[h->cur], sizeof(double) * CAM_IN * h->m, hipMemcpyDeviceToDevice, h->stream));
  h->n_snap++;
  return MVBA_OK;
}

int mvba_snapshot_count(mvba_handle *h, int64_t *n) {
  if (!h || !n) return fail(MVBA_ERR_BADARG, "null argument");
  *n = h->n_snap;
  return MVBA_OK;
}

int mvba_snapshot_read(mvba_handle *h, int64_t i, double *X, double *f, double *u, double *t, double *R) {
  if (!h || !X || !f || !u || !t || !R) return fail(MVBA_ERR_BADARG, "null argument");
  if (i < 0 || i >= h->n_snap) return fail(MVBA_ERR_BADARG, "no such log entry");
  MVBA_HIP(hipSetDevice(h->device));
  const double *src = snap_entry(h, i);
  return read_state(h, src, src + 3 * h->N, X, f, u, t, R);
}

int mvba_snapshot_restore(mvba_handle *h, int64_t i) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  if (i < 0 || i >= h->n_snap) return fail(MVBA_ERR_BADARG, "no such log entry");
  MVBA_HIP(hipSetDevice(h->device));
  const double *src = snap_entry(h, i);
  // what mvba_set_params does, from device memory: the committed state is replaced, linearisation and trial are void
  return write_state(h, src, src + 3 * h->N, hipMemcpyDeviceToDevice);
}

int mvba_snapshot_clear(mvba_handle *h) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  h->n_snap = 0;  // (the slabs stay for the next run; mvba_destroy frees them)
  return MVBA_OK;
}

int mvba_set_profiling(mvba_handle *h, int32_t enabled) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  h->profiling = enabled == 2 ? 2 : (enabled != 0);
  return MVBA_OK;
}

int mvba_get_stats(mvba_handle *h, mvba_stats *out) {
  if (!h || !out) return fail(MVBA_ERR_BADARG, "null argument");
  MVBA_HIP(hipSetDevice(h->device));
  int rc = sync_and_drain(h);
  if (rc) return rc;
  *out = h->stats;
  return MVBA_OK;
}

int mvba_get_info(mvba_handle *h, int64_t *out8) {
  if (!h || !out8) return fail(MVBA_ERR_BADARG, "null argument");
  out8[0] = h->n_items;
  out8[1] = h->n_items_offdiag;
  out8[2] = h->n_units;
  // bits 8..15: the slot form's step width; bit 16: the engine linearises into the compact record; bits 20..27: the slot form's point
  // ranges; bits 28..31: the lane form's wave places per CU as its plan took them; bits 32..: the dense form's workgroups
  out8[3] = h->schur_mode | (h->schur_mode == SCHUR_SLOTS ? h->slot_w << 8 : 0) | (h->rec_compact ? 1 << 16 : 0) |
            (h->schur_mode == SCHUR_SLOTS ? (int64_t)(h->slot_nR & 0xff) << 20 | (int64_t)(h->lane_places & 0xf) << 28 : 0) |
            (h->schur_mode == SCHUR_DENSE ? (int64_t)h->dense_blocks << 32 : 0);
  out8[4] = h->rccl_version;
  out8[5] = NCCL_VERSION_CODE;
  out8[6] = h->nranks;
  out8[7] = h->schur_mode == SCHUR_SLOTS ? h->n_slot_items : 0;  // step-major rows incl. padding
  return MVBA_OK;
}

int mvba_reset_stats(mvba_handle *h) {
  if (!h) return fail(MVBA_ERR_BADARG, "null handle");
  MVBA_HIP(hipSetDevice(h->device));
  int rc = sync_and_drain(h);
  if (rc) return rc;
  h->stats = mvba_stats{};
  return MVBA_OK;
}


}  // extern "C"

// ---- mvba_debug_read
namespace {
// One buffer of mvba_debug_read: its doubles, and the fill of `out` with them (called after a stream synchronisation).
struct DebugBuf {
  long long count = -1;  // -1: no such buffer
  std::function<int(double *)> fill;
};

// `cnt` doubles straight from device memory
DebugBuf debug_copy(const double *src, long long cnt) {
  return {cnt, [=](double *out) -> int {
            MVBA_HIP(hipMemcpy(out, src, sizeof(double) * cnt, hipMemcpyDeviceToHost));
            return MVBA_OK;
          }};
}

// residual, J_X or J_C of every observation: the records expanded on the host
int debug_fill_records(mvba_handle *h, int which, double *out) {
  std::vector<double> r((size_t)2 * REC * h->nobs);
  if (h->rec_compact) {  // ... from the compact ones, the residuals, the committed points and centres (where K1 linearised)
    const size_t no = (size_t)h->nobs;
    std::vector<double> c8(2 * REC_C * no), e2(2 * no), X(3 * (size_t)h->N), cam((size_t)CAM_IN * h->m);
    std::vector<int> pt(no), ck(no);
    MVBA_HIP(hipMemcpy(c8.data(), h->d_rec, sizeof(double) * c8.size(), hipMemcpyDeviceToHost));
    MVBA_HIP(hipMemcpy(e2.data(), h->d_res, sizeof(double) * e2.size(), hipMemcpyDeviceToHost));
    MVBA_HIP(hipMemcpy(X.data(), h->d_X[h->cur], sizeof(double) * X.size(), hipMemcpyDeviceToHost));
    MVBA_HIP(hipMemcpy(cam.data(), h->d_cam15[h->cur], sizeof(double) * cam.size(), hipMemcpyDeviceToHost));
    MVBA_HIP(hipMemcpy(pt.data(), h->d_obs_pt, sizeof(int) * no, hipMemcpyDeviceToHost));
    MVBA_HIP(hipMemcpy(ck.data(), h->d_cam, sizeof(int) * no, hipMemcpyDeviceToHost));
    for (size_t o = 0; o < no; ++o)
      expand_compact_record(&c8[2 * REC_C * o], &e2[2 * o], &X[3 * (size_t)pt[o]], &cam[(size_t)CAM_IN * ck[o] + 3], &r[2 * REC * o]);
  } else
  MVBA_HIP(hipMemcpy(r.data(), h->d_rec, sizeof(double) * r.size(), hipMemcpyDeviceToHost));
  std::vector<double> sw;  // a robust loss: the implied (u, v) columns are sqrt(w) / f0, as the Schur kernels take them
  if (h->loss != LOSS_SQUARED && which == MVBA_BUF_JC) {
    sw.resize(h->nobs);
    MVBA_HIP(hipMemcpy(sw.data(), h->d_sqw, sizeof(double) * sw.size(), hipMemcpyDeviceToHost));
  }
  for (long long o = 0; o < h->nobs; ++o) {
    const double *q = r.data() + (size_t)o * 2 * REC;
    if (which == MVBA_BUF_RESIDUAL) record_to_residual(q, out + 2 * o);
    else if (which == MVBA_BUF_JX) record_to_JX(q, out + 6 * o);
    else record_to_JC(q, sw.empty() ? 1.0 / h->f0 : sw[o] / h->f0, out + 18 * o);
  }
  return MVBA_OK;
}

// `width` doubles from `first` on of every point's row of PL (E_a [6] | dP_a [3])
int debug_fill_point_rows(mvba_handle *h, int first, int width, double *out) {
  std::vector<double> pl(9 * (size_t)h->N);
  MVBA_HIP(hipMemcpy(pl.data(), h->d_PL, sizeof(double) * pl.size(), hipMemcpyDeviceToHost));
  for (long long a = 0; a < h->N; ++a)
    for (int i = 0; i < width; ++i) out[width * a + i] = pl[9 * a + first + i];
  return MVBA_OK;
}

int debug_fill_A(mvba_handle *h, double *out) {  // the packed strips expanded to the dense symmetric matrix
  std::vector<double> pk(h->n_A());
  MVBA_HIP(hipMemcpy(pk.data(), h->d_Ab, sizeof(double) * pk.size(), hipMemcpyDeviceToHost));
  expand_packed_A(pk.data(), h->m, out);
  return MVBA_OK;
}

// the Schur index as the kernel reads it (ints, widened): `cnt` entries of list `which`
int debug_fill_index(mvba_handle *h, int which, long long cnt, double *out) {
  if (h->schur_mode == SCHUR_SLOTS && which != MVBA_BUF_INDEX_SEG) {  // one row per step: k[W] | l[W] | a[W] | pad
    const int W = h->slot_w, row = slot_idx_ints(W);
    const long long n_steps = cnt / W;
    std::vector<int> tmp((size_t)n_steps * row);
    if (cnt) MVBA_HIP(hipMemcpy(tmp.data(), h->d_it_x, sizeof(int) * tmp.size(), hipMemcpyDeviceToHost));
    if (W == LANES_W) {  // two packed words per item: w0[W] | w1[W]
      for (long long st = 0; st < n_steps; ++st)
        for (int sl = 0; sl < W; ++sl) {
          int k, l, a;
          lane_idx_unpack({(unsigned)tmp[(size_t)st * row + sl], (unsigned)tmp[(size_t)st * row + W + sl]}, k, l, a);
          out[st * W + sl] = (double)(which == MVBA_BUF_INDEX_K ? k : (which == MVBA_BUF_INDEX_L ? l : a));
        }
      return MVBA_OK;
    }
    const int off = which == MVBA_BUF_INDEX_K ? 0 : (which == MVBA_BUF_INDEX_L ? W : 2 * W);
    for (long long st = 0; st < n_steps; ++st)
      for (int sl = 0; sl < W; ++sl) out[st * W + sl] = (double)tmp[(size_t)st * row + off + sl];
    return MVBA_OK;
  }
  const int *src = which == MVBA_BUF_INDEX_K ? h->d_it_k : (which == MVBA_BUF_INDEX_L ? h->d_it_l : (which == MVBA_BUF_INDEX_A ? h->d_it_a : h->d_seg_end));
  std::vector<int> tmp((size_t)cnt);
  if (cnt) MVBA_HIP(hipMemcpy(tmp.data(), src, sizeof(int) * tmp.size(), hipMemcpyDeviceToHost));
  for (long long i = 0; i < cnt; ++i) out[i] = (double)tmp[i];
  return MVBA_OK;
}

// THE table of mvba_debug_read's buffers: count and filler of one id
DebugBuf debug_buffer(mvba_handle *h, int which) {
  const long long N = h->N, nobs = h->nobs, n9 = (long long)h->n9();
  switch (which) {
    case MVBA_BUF_RESIDUAL: return {2 * nobs, [=](double *out) { return debug_fill_records(h, which, out); }};
    case MVBA_BUF_JX: return {6 * nobs, [=](double *out) { return debug_fill_records(h, which, out); }};
    case MVBA_BUF_JC: return {18 * nobs, [=](double *out) { return debug_fill_records(h, which, out); }};
    case MVBA_BUF_E: return {6 * N, [=](double *out) { return debug_fill_point_rows(h, 0, 6, out); }};
    case MVBA_BUF_DP: return {3 * N, [=](double *out) { return debug_fill_point_rows(h, 6, 3, out); }};
    case MVBA_BUF_A_FULL: return {n9 * n9, [=](double *out) { return debug_fill_A(h, out); }};
    case MVBA_BUF_B_FULL: return debug_copy(h->d_b(), n9);
    case MVBA_BUF_DXI: return debug_copy(h->d_dxi, n9);
    case MVBA_BUF_DX: return debug_copy(h->d_dX, 3 * N);
    case MVBA_BUF_TRIAL_X: return debug_copy(h->d_X[1 - h->cur], 3 * N);
    case MVBA_BUF_TRIAL_CAM: return debug_copy(h->d_cam15[1 - h->cur], (long long)CAM_IN * h->m);
    case MVBA_BUF_INDEX_K: case MVBA_BUF_INDEX_L: case MVBA_BUF_INDEX_A: case MVBA_BUF_INDEX_SEG: {
      const long long cnt = which == MVBA_BUF_INDEX_SEG ? (h->schur_mode == SCHUR_SLOTS ? (long long)h->n_waves * h->slot_nseg : 0)
                                                        : (h->schur_mode == SCHUR_SLOTS ? h->n_slot_items : (h->schur_mode == SCHUR_PAIRS ? h->n_items : 0));
      return {cnt, [=](double *out) { return debug_fill_index(h, which, cnt, out); }};
    }
    case MVBA_BUF_WEIGHT:
      if (h->loss != LOSS_SQUARED) return debug_copy(h->d_sqw, nobs);
      return {nobs, [=](double *out) { std::fill(out, out + nobs, 1.0); return (int)MVBA_OK; }};
    default: return {};
  }
}
}  // namespace

extern "C" int mvba_debug_read(mvba_handle *h, int32_t which, double *out, int64_t capacity, int64_t *n) {
  if (!h || !n) return fail(MVBA_ERR_BADARG, "null argument");
  MVBA_HIP(hipSetDevice(h->device));
  const DebugBuf buf = debug_buffer(h, which);
  if (buf.count < 0) return fail(MVBA_ERR_BADARG, "unknown buffer id");
  *n = buf.count;
  if (!out) return MVBA_OK;
  if (capacity < buf.count) return fail(MVBA_ERR_BADARG, "output buffer too small");
  MVBA_HIP(hipStreamSynchronize(h->stream));
  return buf.fill(out);
}
