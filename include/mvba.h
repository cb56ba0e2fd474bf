/* mvba.h -- C ABI of libmvba.so: MI355X-native bundle adjustment + factorization SVD.
 *
 * The reference (takah29/3d-reconstruction-from-multi-view-exp) has no FFI layer;
 * the surface it defines is Python:
 *     lib/bundle_adjustment.py:10-206   class BundleAdjuster  (ctor / optimize / get_log)
 *     lib/factorization.py:5-15         factorization_method(W, n_rank)
 * This header is what a ctypes binding underneath those two call sites binds
 * (INTEGRATION.md shows the stub).  The Levenberg-Marquardt control flow
 * (damping schedule, strict accept test, stop rule, log, print; ref :100-195)
 * stays in Python so it is bit-for-bit the reference's; everything that touches
 * observations, points or the reduced camera system is behind these calls.
 *
 * Conventions: every pointer is HOST memory, C-contiguous, little-endian;
 * doubles are IEEE binary64; no struct is passed by value; every function
 * returns an int status (0 = MVBA_OK) and mvba_last_error() gives the
 * thread-local message.  A handle is not thread-safe: one host thread per handle.
 * State (points, cameras) lives in the NORMALISED frame of ref :208-240; the
 * normalise / denormalise transforms are host-side NumPy in lib/bundle_adjustment.py.
 */
#ifndef MVBA_H
#define MVBA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVBA_OK 0
#define MVBA_ERR_BADARG 1   /* -> ValueError              (ref :27-28, :231-232)              */
#define MVBA_ERR_SINGULAR 2 /* -> numpy.linalg.LinAlgError (ref :128 batched inv, :146 solve) */
#define MVBA_ERR_HIP 3      /* -> RuntimeError                                                */
#define MVBA_ERR_RCCL 4     /* -> RuntimeError                                                */
#define MVBA_ERR_STATE 5    /* call order violated (e.g. try_step before linearize)           */

typedef struct mvba_handle mvba_handle;

/* Observation list, CSR by point (replaces the dense x (N,m,2) + bool mask of
 * ref :37, :56-60).  In a point-sharded job n_points / n_obs / pt_ptr describe
 * THIS rank's points; n_images is global (cameras are replicated). */
typedef struct mvba_problem {
  int64_t n_points;       /* points held by this handle                          */
  int64_t n_obs;          /* = pt_ptr[n_points]                                  */
  int32_t n_images;       /* cameras (global)                                    */
  int32_t gauge_axis;     /* 0: "x-right_z-forward" (drops param 12), 1: "x-up_z-forward" (drops 13); ref :62-72 */
  const int64_t *pt_ptr;  /* [n_points+1] offsets into cam_idx / xy              */
  const int32_t *cam_idx; /* [n_obs] camera of each observation, ascending within a point */
  const double *xy;       /* [n_obs][2] observed image coordinates (xy_layout 0) */
  double f0;              /* ref :50                                             */
  int32_t device;         /* HIP device ordinal, -1 = current device             */
  int32_t xy_layout;      /* 0: xy in observation order.  1: xy as image planes [n_images][n_points][2] -- the memory of the
                           * reference caller's np.stack(x_list) (euclidiean_reconstruction.py:50) -- legal only when every point
                           * is observed in every image (n_obs = n_points * n_images; pt_ptr / cam_idx as always); the
                           * observation order is formed on the device instead of by a strided host copy               */
} mvba_problem;

/* Kernel ids for mvba_stats (names via mvba_kernel_name). */
enum {
  MVBA_K_RESID_JAC = 0, /* K1 residual + 2x3 / 2x9 Jacobians   (ref :291-427)            */
  MVBA_K_POINT_BLOCKS,  /* K2 E_a, dP_a (ref :429-469, :519-556): fused into K1, always 0 */
  MVBA_K_POINT_INV,     /* K3a damped 3x3 inverse, E^-1 dP      (ref :120-128)            */
  MVBA_K_SCHUR,         /* K3 A = G^ - sum F^T E^-1 F, b        (ref :132-143, :471-517, :618-664) */
  MVBA_K_ALLREDUCE,     /* C1 RCCL all-reduce of [A|b]                                    */
  MVBA_K_SOLVE,         /* K4 gauge strip + dense solve         (ref :146)                */
  MVBA_K_BACKSUB_COST,  /* K5+K6 dX, trial state, trial cost    (ref :152-162, :260-281, :666-677) */
  MVBA_K_COST,          /* residual-only cost pass              (ref :85-87)              */
  MVBA_K_COUNT
};

typedef struct mvba_stats {
  double ms[16];        /* accumulated device time per kernel id (hipEvents on the library's stream) */
  int64_t launches[16]; /* number of timed launches per kernel id                */
  int64_t n_linearize, n_try_step, n_commit;
  int64_t n_lu_fallback; /* solves that left the Cholesky path for LU with partial pivoting */
  int64_t n_barrier_fallback; /* solves redone with one launch per super-block because a wait of the persistent
                                 back-substitution timed out (its grid was not co-resident)                        */
} mvba_stats;

const char *mvba_version(void);
const char *mvba_last_error(void);
const char *mvba_kernel_name(int32_t kernel_id);
int mvba_device_count(int32_t *count);

/* Copies the observation list to the device and builds the camera-major index. */
int mvba_create(const mvba_problem *problem, mvba_handle **out);
/* The same with a robust loss, fixed for the engine's life.  loss: MVBA_LOSS_*; scale: delta > 0 in image units (pixels).
 * With s = |e|^2 (e in units of x / f0) and b = (delta / f0)^2 the cost is E = sum rho(s):
 *   squared rho = s;  Huber rho = s (s <= b), 2 sqrt(b s) - b;  Cauchy rho = b log1p(s / b).
 * The linearisation is IRLS: every row of an observation is scaled by sqrt(w), w = rho'(s) at the linearisation point.
 * MVBA_LOSS_SQUARED behaves exactly as mvba_create (scale is ignored).  A robust engine never takes the slot form of K3
 * (the unit form instead) and has no covariance (mvba_covariance: MVBA_ERR_BADARG).  MVBA_ERR_BADARG: an unknown loss,
 * or a scale that is not finite and > 0. */
#define MVBA_LOSS_SQUARED 0
#define MVBA_LOSS_HUBER 1
#define MVBA_LOSS_CAUCHY 2
int mvba_create_robust(const mvba_problem *problem, int32_t loss, double scale, mvba_handle **out);
void mvba_destroy(mvba_handle *h);

/* Committed state, normalised frame: X [n_points][3], f [m], u [m][2], t [m][3],
 * R [m][3][3] row-major with COLUMNS = camera axes (ref :40-48).               */
int mvba_set_params(mvba_handle *h, const double *X, const double *f, const double *u,
                    const double *t, const double *R);
int mvba_get_params(mvba_handle *h, double *X, double *f, double *u, double *t, double *R);

/* The way back to the caller's frame, on the device and in place (ref :242-258, applied by the
 * reference's optimize() before it returns, :198-200): X <- scale X R0^T + t0, t likewise,
 * R <- R0 R on the committed state.  R0 [3][3] row-major, t0 [3]. */
int mvba_apply_similarity(mvba_handle *h, const double *R0, const double *t0, double scale);

/* E = sum over observations of |e|^2 at the committed state (ref :666-677). */
int mvba_cost(mvba_handle *h, double *E);
/* K1+K2 at the committed state (ref :103-116). */
int mvba_linearize(mvba_handle *h);
/* One LM trial with damping c (ref :118-162): K3a,K3,(C1),K4,K5,K6; the trial
 * state stays on the device.  *E_trial is the job-wide cost at the trial state. */
int mvba_try_step(mvba_handle *h, double c, double *E_trial);
/* trial -> committed (ref :169-173). */
int mvba_commit(mvba_handle *h);

/* Parameter map: which camera parameters a trial adjusts.  Parameter p of camera k is slot g = 9 k + p, p in the order
 * f, u, v, t[3], omega[3] (the order of MVBA_BUF_DXI).  col [9 n_images]: -1 holds slot g (its increment is 0 in every
 * step); j in 0 .. n_free-1 makes it the reduced unknown j, and slots with the same j are TIED (they get the same
 * increment).  With P[g][col g] = 1 a trial solves (P^T A P) x = P^T b on the reduced camera system [A | b] it solves
 * today and steps by dxi = P x; everything else is unchanged.  NULL restores the default map: the seven gauge slots (camera
 * 0's t and omega, component gauge_axis of camera 1's t) held, all others free in ascending order, n_free = 9 n_images - 7.
 * Rules (MVBA_ERR_BADARG, the message names the offending index): the gauge slots are -1; -1 <= col[g] < n_free; every
 * unknown has a slot; tied slots are the same intrinsic parameter (p <= 2) of different cameras.  n_free = 0 is legal: the
 * cameras stay, the points move by -E_a^-1 dP_a, no dense solve runs.  The caller gives tied parameters equal values; equal
 * increments then keep them equal bit for bit.  May be called any time after mvba_create; keeps the linearisation, voids
 * the trial (mvba_commit before the next mvba_try_step is MVBA_ERR_STATE).  mvba_covariance honours the map: Cov = P Sigma'
 * P^T, zero rows and columns where held.  Sharded: every rank must set the same map (it acts after the all-reduce). */
int mvba_set_parameter_map(mvba_handle *h, const int32_t *col, int32_t n_free);

/* Held points: which points a trial adjusts.  held [n_points], nonzero = point a is not an unknown; NULL (or no nonzero
 * entry) clears the mask.  A trial then solves the problem in the remaining 3 (n_points - n_held) + n_free unknowns: the
 * normal equations with the held points' columns deleted and the same damping (1 + c) on the diagonals that remain.  K3a
 * writes E_a^-1 = 0, v_a = 0 for a held point, so its -F^T E^-1 F terms vanish from the reduced camera system, b keeps its
 * -2 Jc^T e term, and dX_a = 0: MVBA_BUF_DX is 0 and MVBA_BUF_TRIAL_X equals the committed X there, bit for bit.  The cost,
 * the residuals and the robust weights run over every observation, those of held points included; MVBA_BUF_E /
 * MVBA_BUF_DP stay the undamped sums they are.  E_a of a held point is never inverted: a held point seen once, or without
 * parallax, is legal (MVBA_ERR_SINGULAR is for free points only).  Holding is per whole point, and in the frame the
 * engine's state is in (the seven gauge slots stay held whatever the mask: holding three or more points does not free
 * them).  May be called any time after mvba_create; keeps the linearisation, voids the trial (mvba_commit before the next
 * mvba_try_step is MVBA_ERR_STATE).  Independent of the parameter map and of the loss.  mvba_covariance honours the mask:
 * six zeros for a held point, no pivot test for it, and the camera blocks of the problem with those points fixed.
 * mvba_triangulate_state with a mask set is MVBA_ERR_STATE: clear the mask first (a held point is not re-triangulated
 * silently).  Sharded: the mask covers this rank's points, nothing is communicated.  Without a mask the engine issues the
 * launches it issues today. */
int mvba_set_point_hold(mvba_handle *h, const uint8_t *held);

/* Marginal covariances at the COMMITTED state, undamped, gauge parameters fixed (zero rows/columns): the unit covariance
 * C = (J^T J)^-1 = 2 H^-1 over the free parameters (J: the residual Jacobian, units x / f0), camera parameters in the order
 * f, u, v, t[3], omega[3].  Runs K1, K3a at c = 0, the engine's K3 form, the all-reduce of [A|b] and K4's Cholesky, then
 * S^-1 from the factor and one point-major pass.
 * point_cov [n_points][6] (xx,xy,xz,yy,yz,zz), cam_cov [m][9][9], cam_cov_full [9m][9m]: each may be NULL.
 * timings_ms [4] (may be NULL): linearise+Schur, factor, inverse, point pass.  Afterwards the handle is as
 * mvba_linearize leaves it (no trial); the committed parameters are untouched.  MVBA_ERR_SINGULAR: a non-positive pivot of
 * the undamped reduced camera system, or a numerically singular point block E_a (a Cholesky pivot below 1e-12 of its largest
 * diagonal entry: a point seen once) of a point that is not held (mvba_set_point_hold).  Sharded: every rank gets its own points' blocks and the same camera blocks.        */
int mvba_covariance(mvba_handle *h, double *point_cov, double *cam_cov, double *cam_cov_full, double *timings_ms);

/* e [n_obs][2]: f0 e_o, the residual of every observation in image units at the COMMITTED state, in the engine's
 * observation order (this rank's observations when sharded).  Independent of the loss. */
int mvba_residuals(mvba_handle *h, double *e);

/* The debug log of the reference's optimize(is_debug=True) (ref :89-98, :175-183: a copy of X, R, t per outer
 * iteration, normalised frame; read back by get_log(), :204-206).  mvba_snapshot appends the COMMITTED state to
 * a log kept in device memory -- one device-to-device copy on the engine's stream, nothing crosses PCIe and the
 * host does not wait; mvba_snapshot_read fetches entry i (what get_log() does, once, afterwards);
 * mvba_snapshot_clear empties the log (the reference clears it at the start of every optimize, :90) and keeps
 * its memory for the next run; mvba_snapshot_restore makes entry i the committed state again (mvba_set_params
 * from device memory: linearisation and trial become void; nothing crosses PCIe). */
int mvba_snapshot(mvba_handle *h);
int mvba_snapshot_count(mvba_handle *h, int64_t *n);
int mvba_snapshot_read(mvba_handle *h, int64_t i, double *X, double *f, double *u, double *t, double *R);
int mvba_snapshot_clear(mvba_handle *h);
int mvba_snapshot_restore(mvba_handle *h, int64_t i);

/* Per-kernel device timing (hipEvents on the engine's stream); off by default.  enabled = 1: every phase;
 * 2: the Schur (K3) and residual-Jacobian (K1) kernels only -- each timed phase is two marker packets on the stream. */
int mvba_set_profiling(mvba_handle *h, int32_t enabled);
int mvba_get_stats(mvba_handle *h, mvba_stats *out);
int mvba_reset_stats(mvba_handle *h);

/* Sizes of the Schur index built at create and what the communicator runs on (bench.py prices the
 * kernels with them): out[0] (point, camera pair) items incl. diagonal pairs, out[1] off-diagonal
 * items, out[2] units (wave runs / slot lists), out[3] Schur kernel form (0, round 1's camera strips, is no longer produced):
 * 1 = pair-major units (round 2), 2 = slot-resident (round 3), 3 = dense visibility (round 5: at most 21 cameras and at least
 * 60 % of the (point, camera) pairs observed: no pair index, out[0..2] = 0) in bits 0..7; bits 8..15: the slot form's step
 * width = lists per wave (21: three lanes per item, 64: one lane per item; 0 in the other forms); bit 16: the engine linearises
 * into the compact 64-byte record (lane form, squared loss, at most 646 cameras, not MVBA_REC=full); bits 32..63: the dense form's
 * launch, the workgroups of k_schur_dense = min(chunks of points, CUs x workgroups per CU) (0 in the other forms), out[4] ncclGetVersion() of the librccl
 * actually loaded (0 without a communicator), out[5] the NCCL_VERSION_CODE the library was compiled
 * against, out[6] ranks, out[7] slot form: step-major item rows including the padding rows. */
int mvba_get_info(mvba_handle *h, int64_t *out8);

/* Point-sharded multi-GPU (one process per GPU): rank 0 makes an id, the host
 * side ships its 128 bytes to the other ranks, every rank calls comm_init.
 * Afterwards try_step all-reduces the partial reduced system [A|b] over RCCL and
 * cost / try_step return the sum of the ranks' costs taken in rank order.      */
int mvba_comm_unique_id(void *id128);
int mvba_comm_init(mvba_handle *h, const void *id128, int32_t rank, int32_t n_ranks);

/* The same sharded job over a HOST-STAGED transport instead of RCCL: the library copies the packed
 * [A|b] (and the 16-byte cost/status record) to the host and calls `fn(user, buf, n)`, which must
 * sum `buf` in place over all ranks (e.g. a gloo / MPI all-reduce) and return 0.  For machines
 * without RCCL and for multi-process tests that share one GPU (RCCL refuses two ranks on one
 * device); control flow, rank-ordered cost sum and collective error behaviour are identical. */
typedef int (*mvba_host_allreduce_fn)(void *user, double *buf, int64_t n);
int mvba_comm_init_host(mvba_handle *h, int32_t rank, int32_t n_ranks, mvba_host_allreduce_fn fn, void *user);

/* Test hook: download an intermediate in canonical per-observation / per-point
 * row-major layout.  Returns the element count in *n (out may be NULL to query). */
enum {
  MVBA_BUF_RESIDUAL = 0, /* [n_obs][2]                                       */
  MVBA_BUF_JX,           /* [n_obs][2][3]                                    */
  MVBA_BUF_JC,           /* [n_obs][2][9]                                    */
  MVBA_BUF_E,            /* [n_points][6]  xx,xy,xz,yy,yz,zz  (undamped)     */
  MVBA_BUF_DP,           /* [n_points][3]                                    */
  MVBA_BUF_A_FULL,       /* [9m][9m] symmetric, before gauge removal         */
  MVBA_BUF_B_FULL,       /* [9m]                                             */
  MVBA_BUF_DXI,          /* [9m] with zeros at the gauge slots (with a map: where held; equal where tied) */
  MVBA_BUF_DX,           /* [n_points][3]  (0 at held points)                */
  MVBA_BUF_TRIAL_X,      /* [n_points][3]  (the committed X at held points)  */
  MVBA_BUF_TRIAL_CAM,    /* [m][15]  f,u,v,t[3],R[9]                         */
  MVBA_BUF_INDEX_K,      /* the Schur index as the kernel reads it: k-side observation of every item row */
  MVBA_BUF_INDEX_L,      /*   l-side observation                                                          */
  MVBA_BUF_INDEX_A,      /*   point (slot form: step-major rows incl. padding; unit form: pair-major)      */
  MVBA_BUF_INDEX_SEG,    /*   slot form: pacing table [waves][segments]                                   */
  MVBA_BUF_WEIGHT        /* [n_obs] sqrt(w_o) of the last linearisation (robust loss; 1 for the squared loss)   */
};
/* (robust loss: RESIDUAL, JX and JC are the rows as K3 sees them -- scaled by sqrt(w_o), the implied (u, v) columns
 * of JC sqrt(w_o) / f0) */
int mvba_debug_read(mvba_handle *h, int32_t which, double *out, int64_t capacity, int64_t *n);

/* Pinhole projection of an observation list on the device: xy[o] = inhomogeneous
 * K_k [R_k^T | -R_k^T t_k] [X_a; 1] (ref lib/camera.py:13-14, :30-34, :74-81 -- the scene side of
 * BA: synthetic observations before it, re-projection after it).  K, R [n_images][3][3] row-major
 * (R: columns = camera axes), t [n_images][3].  pt_ptr / cam_idx as in mvba_problem; pt_ptr == NULL
 * means the dense grid (n_obs = n_points * n_images, observation = point * n_images + camera: the
 * reference's calc_projected_points, transposed).  xy [n_obs][2] is written. */
int mvba_project(const double *X, int64_t n_points, const double *K, const double *R, const double *t, int32_t n_images,
                 const int64_t *pt_ptr, const int32_t *cam_idx, int64_t n_obs, double *xy, int32_t device);

/* ---- initial estimates (csrc/mvba_init.h): the two steps that extend a reconstruction ---------------
 * mvba_triangulate: every point from known cameras, the inverse of mvba_project on noise-free data.  K, R, t, pt_ptr,
 * cam_idx, xy mean what they mean there (P_k = K_k [R_k^T | -R_k^T t_k] formed in k_project_obs's order of operations,
 * xy = (p0 / p2, p1 / p2): xy is in the units K projects to -- for raw image coordinates and the engine's f, u that is
 * K[2][2] = 1, not f0 --); pt_ptr == NULL is the dense grid; the same argument checks (MVBA_ERR_BADARG, the message
 * gives the offending number) and the same LDS camera table: at most 1704 cameras.
 * Per point a, observations o in ascending order: the rows x_o P[2] - P[0] and y_o P[2] - P[1], each scaled to unit
 * length, M_a = sum row^T row (4 x 4), X~ = the eigenvector of its smallest eigenvalue, X = X~[:3] / X~[3]; then n_refine
 * >= 0 Gauss-Newton steps on sum_o |pi(P_k X) - xy_o|^2 (3 x 3 normal equations, Cholesky), a step taken only if it does
 * not raise the point's cost, otherwise the point stops.
 * status [n_points]: 0 ok; 1 fewer than two observations; 2 no parallax (second-smallest eigenvalue of M_a <= 1e-12 x the
 * largest, the relative pivot rule of mvba_covariance); 3 at infinity (|X~[3]| <= 1e-12 |X~|) or a result that is not
 * finite.  Where status != 0, X and quality are NaN.
 * quality [n_points][3]: RMS reprojection residual at the returned X in units of xy; the smallest depth
 * (R_k^T (X - t_k))_z over the point's cameras (<= 0: behind a camera); the largest angle in radians between two of the
 * point's viewing rays (all pairs: deg^2 / 2 per point, skipped when quality is NULL).
 * timings_ms [3]: upload, kernel, download.  quality, status, timings_ms may each be NULL.  One thread per point, sums in
 * ascending observation order, no atomics: two calls give bitwise-identical output. */
int mvba_triangulate(const double *K, const double *R, const double *t, int32_t n_images, int64_t n_points, const int64_t *pt_ptr,
                     const int32_t *cam_idx, const double *xy, int64_t n_obs, int32_t n_refine, double *X, double *quality,
                     int32_t *status, double *timings_ms, int32_t device);
/* The same on the observations and the COMMITTED cameras the engine already holds (nothing is uploaded), with the BA
 * camera model K = [[f,0,u],[0,f,v],[0,0,f0]] (which projects to x / f0; the engine's xy are the caller's x, so the rows are
 * formed with the third row divided by f0, K[2][2] = 1: the same solution, and quality[0] is in the units of xy for any f0):
 * replaces the committed points; a point with status != 0 keeps its old
 * coordinates.  Voids the linearisation and the trial, as mvba_set_params does.  Independent of the loss.  Sharded: each
 * rank does its own points, nothing is communicated.  MVBA_ERR_STATE before the first mvba_set_params, and while a point
 * mask is set (mvba_set_point_hold: clear it first); MVBA_ERR_BADARG above 1704 cameras. */
int mvba_triangulate_state(mvba_handle *h, int32_t n_refine, double *quality, int32_t *status, double *timings_ms);
/* mvba_resect: every camera from known points, the normalised DLT.  X [n_points][3]; the list as in mvba_project (pt_ptr ==
 * NULL: the dense grid); point_ok [n_points] != 0 marks the points to use (NULL: those whose X is finite).
 * The list is sorted camera-major on the host (a stable counting sort, ascending points inside a camera) and cut into chunks
 * of 256 observations.  Device pass 1: per camera the count, centroid and mean squared distance of its 3-D points and of its
 * image points (Hartley: scaled to mean squared distance 3 and 2).  Device pass 2: N_k = sum row^T row of the normalised DLT
 * rows [X~^T, 0, -x X~^T], [0, X~^T, -y X~^T] -- its 78 unique entries are the 40 sums of (1, x, y, x^2 + y^2) X~ X~^T --
 * a chunk by a fixed tree, the chunks of a camera in ascending order: two runs are bitwise equal.  The eigenvector of the
 * smallest eigenvalue (cyclic Jacobi on the host: n_images problems of order 12), the two normalisations undone:
 * P [n_images][12] row-major 3 x 4 (it projects to the units of the xy given), scaled so that |P[2][:3]| = 1 and det P[:, :3] > 0.
 * status [n_images]: 0 ok; 1 fewer than 6 usable observations; 2 degenerate, e.g. coplanar points (second-smallest
 * eigenvalue <= 1e-12 x the largest).  Where status != 0, P is NaN.
 * quality [n_images][2]: RMS reprojection residual of the camera's used observations (a third device pass; NaN where status
 * != 0); the eigenvalue ratio lambda_1 / lambda_2 (small: well determined; NaN where status = 1, and where the
 * sums are not finite: points or image points that coincide exactly make a Hartley scale infinite, status 2).
 * timings_ms [3]: sort + upload, kernels, everything else (copies back, eigen-solves).  quality, status, timings_ms may be NULL. */
int mvba_resect(const double *X, int64_t n_points, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy, int64_t n_obs,
                int32_t n_images, const uint8_t *point_ok, double *P, double *quality, int32_t *status, double *timings_ms,
                int32_t device);

/* mvba_covisibility: count [n_images][n_images], count[k][l] = the number of points observed in both k and l (symmetric),
 * count[k][k] = camera k's observation count.  The list as in mvba_project (pt_ptr == NULL: the dense grid, cam_idx unused); the
 * argument checks and the camera cap (1704) are mvba_triangulate's.  One thread per point walks the pairs of its own camera run
 * (deg^2 / 2 per point) into integer counters: exact in any order.  timings_ms [3] (may be NULL): upload, kernel, everything else. */
int mvba_covisibility(int64_t n_points, int32_t n_images, const int64_t *pt_ptr, const int32_t *cam_idx, int64_t n_obs,
                      int64_t *count, double *timings_ms, int32_t device);

/* mvba_two_view: the fundamental matrix of each requested camera pair from the points the two cameras share: the normalised
 * 8-point method.  The list as in mvba_project (pt_ptr == NULL: the dense grid) with cam_idx strictly ascending within a point
 * (MVBA_ERR_BADARG otherwise); xy [n_obs][2] in any units.  pairs [n_pairs][2] = (k, l), k != l.  For pair (k, l) the shared
 * points are those with an observation in both images, in ascending point order; x_k, x_l are a shared point's two observations.
 * Device pass 1: the count n, and per side the centroid c and the mean squared distance d to it (Hartley: x~ = s (x - c) with
 * s = sqrt(2) / sqrt(d), mean squared distance 2 -- mvba_resect's convention for image points).  Device pass 2: M = sum a a^T
 * of the rows a = (x~_l x~_k, x~_l y~_k, x~_l, y~_l x~_k, y~_l y~_k, y~_l, x~_k, y~_k, 1), its 45 unique sums -- a chunk of 256
 * points by a fixed tree, a pair's chunks in an order the chunk count fixes, no floating-point atomics: two runs are bitwise
 * equal.  Host: F^ (3 x 3 row-major) = the eigenvector of M's smallest eigenvalue (cyclic Jacobi, n_pairs problems of order 9),
 * so that x~_l^T F^ x~_k = 0; rank 2 by zeroing F^'s smallest singular value; F = T_l^T F^ T_k with
 * T = [[s, 0, -s c_x], [0, s, -s c_y], [0, 0, 1]]; scaled to Frobenius norm 1 with its largest-magnitude entry positive.
 * F [n_pairs][9]: x_l^T F x_k = 0 in the units of xy.
 * status [n_pairs]: 0 ok; 1 fewer than 8 shared points; 2 degenerate (second-smallest eigenvalue of M <= 1e-12 x the largest:
 * noise-free points in a plane, two cameras at one centre).  Where status != 0, F and quality are NaN.
 * quality [n_pairs][2]: the RMS Sampson distance of the shared points under the returned F, in the units of xy (a third device
 * pass; squared distance (x_l^T F x_k)^2 / ((F x_k)_0^2 + (F x_k)_1^2 + (F^T x_l)_0^2 + (F^T x_l)_1^2)); lambda_1 / lambda_2
 * of M (small: well determined).  n_shared [n_pairs]: the count.
 * timings_ms [3]: check + upload, kernels, everything else (copies back, eigen-solves).  quality, n_shared, status and
 * timings_ms may be NULL.  MVBA_ERR_BADARG (with the number in the message): a pair with k == l or an index outside
 * 0 .. n_images - 1, n_pairs < 0, and whatever mvba_triangulate rejects of a list. */
int mvba_two_view(int64_t n_points, int32_t n_images, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy,
                  int64_t n_obs, const int32_t *pairs, int32_t n_pairs, double *F, double *quality, int64_t *n_shared,
                  int32_t *status, double *timings_ms, int32_t device);

/* mvba_two_view_robust: mvba_two_view with 8-point RANSAC in front of it.  The list, pairs, argument checks, camera cap and
 * error messages are mvba_two_view's; further MVBA_ERR_BADARG (with the number in the message): threshold not finite or not
 * > 0, n_hypotheses outside 1 .. 65536, n_refit outside 0 .. 16.  Per pair (k, l), the shared points in ascending point
 * order numbered 0 .. n - 1 (compacted on the device into a dense array):
 *   normalisation: centroids and Hartley scales over ALL shared points, as mvba_two_view defines them;
 *   hypothesis h = 0 .. n_hypotheses - 1: the 8 distinct indices of mvba_ransac_sample(seed, k, l, h, n); M_h = sum a a^T over
 *     their 8 normalised rows (mvba_two_view's row); F^_h = the eigenvector of its smallest eigenvalue (cyclic Jacobi on the
 *     device); degenerate if lambda_2 <= 1e-12 lambda_max or anything is not finite; F_h = T_l^T F^_h T_k, no rank-2 step;
 *   score: count_h = the number of shared points with squared Sampson distance (mvba_two_view's) <= threshold^2 under F_h, an
 *     integer (ballots and integer atomics: exact in any order); -1 for a degenerate hypothesis; best = the largest count, the
 *     lowest h on ties;
 *   refit r = 1 .. n_refit: the full mvba_two_view fit (its own normalisation, fixed-order sums, the eigen-problem, the rank-2
 *     step and the scaling on the host) on the current inlier set alone, I_0 being that of F_best; I_r = the points within the
 *     threshold of that F.  A refit is kept if its status is 0 and |I_r| >= |I_r-1|; otherwise the loop stops with the
 *     previous result.  If none is kept (n_refit = 0 too) F is F^_best made rank 2, denormalised and scaled by the same host step.
 * F [n_pairs][9]: |F| = 1, largest-magnitude entry positive.  quality [n_pairs][2]: the RMS Sampson distance over the final
 * inliers under the matrix that selected them (the last kept refit's F; F_best itself if none was kept), and lambda_1 /
 * lambda_2 of the last kept refit (0 if none: a minimal sample's M has rank 8).  n_shared, n_inliers, best [n_pairs] (best =
 * -1 where status = 1 or 2).  inlier [n_pairs][n_points] (n_pairs x n_points BYTES): 1 where the point is a final inlier of the pair.
 * hyp_count [n_pairs][n_hypotheses]: the count table (all -1 where status = 1).
 * status [n_pairs]: 0 ok; 1 fewer than 8 shared points; 2 every hypothesis degenerate (or the host step failed); 4 the best
 * count is below 8.  Where status != 0, F and quality are NaN, n_inliers is 0 and the mask is 0.
 * timings_ms [4]: check + upload; compaction, normalisation, hypotheses and scoring; refits; everything else (host clock, each
 * phase ends in a blocking copy).  Every output but F may be NULL.  Pairs are taken in tiles of
 * 128 MiB / (48 n_points + 160 n_hypotheses), at most 65535.  Two calls give bitwise-identical output. */
int mvba_two_view_robust(int64_t n_points, int32_t n_images, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy,
                         int64_t n_obs, const int32_t *pairs, int32_t n_pairs, double threshold, int32_t n_hypotheses,
                         uint64_t seed, int32_t n_refit, double *F, double *quality, int64_t *n_shared, int64_t *n_inliers,
                         int32_t *best, uint8_t *inlier, int32_t *hyp_count, int32_t *status, double *timings_ms, int32_t device);
/* Host only (no GPU needed): the 8 distinct indices below n that hypothesis h of pair (k, l) draws -- the function the kernel
 * runs.  mix(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB;
 * x ^ x >> 31.  s = mix(mix(mix(seed) ^ (k << 32 | l)) ^ h); repeat s = mix(s), j = ((s >> 32) * n) >> 32, keep j unless
 * already drawn.  MVBA_ERR_BADARG: n outside 8 .. 2^31 - 1, a negative k, l or h. */
int mvba_ransac_sample(uint64_t seed, int32_t k, int32_t l, int32_t h, int64_t n, int64_t *idx8);

/* mvba_homography_robust: the homography of each pair, x_l ~ H x_k in the units of xy, by 4-point RANSAC -- the model for points
 * in a plane (and for two cameras at one centre), where the fundamental matrix is not determined.  The argument list, the
 * checks, the compaction, the normalisation over all shared points, the count table, the refit loop and the tiles are
 * mvba_two_view_robust's (one host loop and one set of scoring, mask and refit kernels serve both); H stands where F stands.
 *   hypothesis h: the 4 indices of mvba_homography_sample(seed, k, l, h, n); the homography of the four normalised
 *     correspondences in closed form, in registers: per image B = [l1 p1, l2 p2, l3 p3] with [p1 p2 p3] l = p4 (p = (x, y, 1);
 *     Cramer's rule), H^ = B_l adj(B_k), H^^-1 ~ B_k adj(B_l); degenerate if one of the four point triples of either image has
 *     |det [p_a p_b p_c]| <= 1e-12 |p_a| |p_b| |p_c|, or an entry is not finite; H = T_l^-1 H^ T_k and its inverse likewise;
 *   inlier test, without a division: with (u, v, w) = H (x_k, y_k, 1): w > 0 and (u - x_l w)^2 + (v - y_l w)^2 <= threshold^2 w^2,
 *     and the same with H^-1 from l to k.  The sign of a matrix matters to w > 0: H and H^-1 each carry the sign that makes w
 *     positive at the centroid of the points they are applied to (of all shared points for a hypothesis, of the fitted inliers
 *     for a refit);
 *   refit: the normalised DLT on the current inliers -- the 45 moments of the two rows per correspondence, the order-9
 *     eigen-problem on the host, degenerate if lambda_2 <= 1e-12 lambda_max; no rank step; H^-1 for its mask pass is adj(H).
 *     Kept while the inlier set does not shrink.  If none is kept, H is the best hypothesis's as the sample gives it.
 * H [n_pairs][9]: |H|_F = 1, largest-magnitude entry positive.  quality [n_pairs][2]: the RMS of the inliers' symmetric transfer
 * distance sqrt(mean((d_kl^2 + d_lk^2) / 2)) under the matrix that selected them; lambda_1 / lambda_2 of the last kept refit (0 if
 * none).  status [n_pairs]: 0 ok; 1 fewer than 4 shared points; 2 every hypothesis degenerate (collinear points); 4 the best
 * count is below 4.  Tiles: 128 MiB / (48 n_points + 160 n_hypotheses) pairs.  Two calls give bitwise-identical output. */
int mvba_homography_robust(int64_t n_points, int32_t n_images, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy,
                           int64_t n_obs, const int32_t *pairs, int32_t n_pairs, double threshold, int32_t n_hypotheses,
                           uint64_t seed, int32_t n_refit, double *H, double *quality, int64_t *n_shared, int64_t *n_inliers,
                           int32_t *best, uint8_t *inlier, int32_t *hyp_count, int32_t *status, double *timings_ms, int32_t device);
/* Host only (no GPU needed): the 4 distinct indices below n that hypothesis h of pair (k, l) draws -- the first 4 of
 * mvba_ransac_sample(seed, k, l, h, n) wherever n >= 8.  MVBA_ERR_BADARG: n outside 4 .. 2^31 - 1, a negative k, l or h. */
int mvba_homography_sample(uint64_t seed, int32_t k, int32_t l, int32_t h, int64_t n, int64_t *idx4);

/* mvba_resect_robust: mvba_resect with 6-point RANSAC in front of it.  X, the list, point_ok, the usable-observation rule and
 * the camera-major stable counting sort with chunks of 256 observations are mvba_resect's.  cameras [n_cameras]: the cameras to
 * solve (NULL: all of them, n_cameras = n_images); duplicates are legal; every per-camera output is indexed by the position in
 * cameras.  MVBA_ERR_BADARG (with the number in the message): a camera index outside 0 .. n_images - 1, n_cameras < 0,
 * threshold not finite or not > 0, n_hypotheses outside 1 .. 65536, n_refit outside 0 .. 16, and whatever mvba_resect rejects.
 * Per listed camera k, its usable observations in ascending point order numbered 0 .. n - 1 (a dense run after the sort):
 *   normalisation: centroids and Hartley scales over ALL usable observations, as mvba_resect defines them;
 *   hypothesis h = 0 .. n_hypotheses - 1: the 6 distinct indices of mvba_resect_sample(seed, k, h, n); the 12 x 12 moment
 *     matrix of their 12 normalised DLT rows, from the 40 sums as in mvba_resect; p^_h = the eigenvector of its smallest
 *     eigenvalue (cyclic Jacobi on the device); degenerate if lambda_2 <= 1e-12 lambda_max or anything is not finite; P_h = p^_h
 *     denormalised and scaled to |P[2][:3]| = 1, det P[:, :3] > 0;
 *   score: count_h = the number of usable observations with depth P[2] . (X, 1) > 0 and squared reprojection distance
 *     |pi(P X) - xy|^2 <= threshold^2 under P_h, an integer (ballots and integer atomics: exact in any order); -1 for a
 *     degenerate hypothesis; best = the largest count, the lowest h on ties;
 *   refit r = 1 .. n_refit: the full mvba_resect fit (its own normalisation, fixed-order sums under a byte mask, the order-12
 *     eigen-problem on the host) on the current inlier set alone, I_0 being that of P_best; I_r = the observations within the
 *     threshold and in front of that P.  Refit 1 is kept if its status is 0 and |I_1| >= 6; refit r >= 2 if its status is 0
 *     and |I_r| >= |I_r-1|; otherwise the loop stops with the previous result.  (Not mvba_two_view_robust's rule: a minimal
 *     6-point DLT is far worse conditioned than a minimal 8-point F, and its count is no bar for the full fit.)  With
 *     n_refit = 0, P is P_best.
 * P [n_cameras][12].  quality [n_cameras][2]: the RMS reprojection residual over the final inliers under the matrix that
 * selected them; lambda_1 / lambda_2 of the last kept refit (0 if none).  n_usable, n_inliers, best [n_cameras] (best = -1
 * where status = 1 or 2).  inlier [n_obs] BYTES in the caller's observation order: 1 for a final inlier of a listed camera of
 * status 0, 0 elsewhere.  hyp_count [n_cameras][n_hypotheses]: the count table (all -1 where status = 1 or 2).
 * status [n_cameras]: 0 ok; 1 fewer than 6 usable observations; 2 every hypothesis degenerate; 4 the best count is below 6.
 * Where status != 0, P and quality are NaN and n_inliers is 0.
 * timings_ms [4]: sort + upload; normalisation, hypotheses and scoring; refits; everything else (host clock, each phase ends in
 * a blocking copy).  Every output but P may be NULL.  Cameras are taken in tiles of 128 MiB / (100 n_hypotheses), at least 1
 * and at most 65535; a camera's results do not depend on which other cameras are listed.  Two calls give bitwise-identical output. */
int mvba_resect_robust(const double *X, int64_t n_points, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy,
                       int64_t n_obs, int32_t n_images, const uint8_t *point_ok, const int32_t *cameras, int32_t n_cameras,
                       double threshold, int32_t n_hypotheses, uint64_t seed, int32_t n_refit, double *P, double *quality,
                       int64_t *n_usable, int64_t *n_inliers, int32_t *best, uint8_t *inlier, int32_t *hyp_count, int32_t *status,
                       double *timings_ms, int32_t device);
/* Host only (no GPU needed): the 6 distinct indices below n that hypothesis h of camera k draws -- mvba_ransac_sample's
 * generator with l = k and 6 draws: the first 6 of mvba_ransac_sample(seed, k, k, h, n) wherever n >= 8.  MVBA_ERR_BADARG: n
 * outside 6 .. 2^31 - 1, a negative k or h. */
int mvba_resect_sample(uint64_t seed, int32_t k, int32_t h, int64_t n, int64_t *idx6);

/* mvba_pose_robust: the poses of cameras with KNOWN intrinsics from known points -- three-point (P3P) RANSAC, then a pose-only
 * Gauss-Newton refit on the inliers (csrc/mvba_pose_ransac.h).  X, the list, point_ok, cameras / n_cameras,
 * threshold, n_hypotheses, seed, n_refit and device are mvba_resect_robust's, with the same checks and messages; K
 * [n_images][3][3] projects to the units of xy (the conventions of mvba_project: x ~ K R^T (X - t)); n_refine in 0 .. 16
 * (MVBA_ERR_BADARG with the number in the message otherwise, as for a NULL K).
 * Per listed camera k, its usable observations in ascending point order numbered 0 .. n - 1 (a dense run after the sort):
 *   hypothesis h = 0 .. n_hypotheses - 1: the 4 distinct indices (i0, i1, i2, i3) of mvba_pose_sample(seed, k, h, n); bearings
 *     d_j = K^-1 (x, y, 1) scaled to unit length (K inverted by its adjugate); a = |X_1 - X_2|, b = |X_0 - X_2|, c = |X_0 - X_1|,
 *     cos alpha = d_1 . d_2, cos beta = d_0 . d_2, cos gamma = d_0 . d_1; the depths s > 0 with s_1^2 + s_2^2 - 2 s_1 s_2 cos alpha
 *     = a^2, s_0^2 + s_2^2 - 2 s_0 s_2 cos beta = b^2, s_0^2 + s_1^2 - 2 s_0 s_1 cos gamma = c^2: with u = s_1 / s_0, v = s_2 / s_0,
 *     q = (a^2 - c^2) / b^2, W = 1 + v^2 - 2 v cos beta: u = (q W - v^2 + 1) / (2 (cos gamma - v cos alpha)), a quartic in v from
 *     the third equation, s_0^2 = b^2 / W.  The quartic's real roots: monic and depressed (y^4 + p y^2 + g y + h), Ferrari's two
 *     quadratics y^2 +- sqrt(2 m) y + p / 2 + m -+ g / (2 sqrt(2 m)) with m a positive root of m^3 + p m^2 + (p^2 / 4 - h) m -
 *     g^2 / 8 (50 steps from the bracket 0 .. 1 + the largest coefficient magnitude, starting at its upper end: Newton's step
 *     where it stays inside the bracket, the midpoint where it does not), a quadratic's two roots where its
 *     discriminant is >= 0, each polished by 2 Newton steps on the quartic.  Every root with u, v, s_0 > 0 gets 3 Newton steps on
 *     the three equations (a 3 x 3 solve) and is dropped unless the depths are positive and finite afterwards.  Its pose: Y_j =
 *     s_j d_j; the orthonormal frames of the triangles (Y_0, Y_1, Y_2) and (X_0, X_1, X_2) by Gram-Schmidt (e_1 along 1 - 0, e_2
 *     along 2 - 0 without its e_1 part, e_3 = e_1 x e_2); R_cw = F_Y F_X^T, R = R_cw^T, t = X_0 - R Y_0.  The hypothesis's pose is
 *     the solution that puts X_i3 in front of the camera with the smallest squared reprojection distance at observation i3
 *     (the smaller s_0 on a tie).  Degenerate (count -1): no such solution, anything not finite, or a triangle whose e_2
 *     remainder has squared length <= 1e-12 x that of its 2 - 0 edge;
 *   score: P_h = K [R^T | -R^T t]; count_h = the number of usable observations in front of P_h and within threshold^2 of it --
 *     the test and the kernel of mvba_resect_robust --; best = the largest count, the lowest h on ties (on the host);
 *   refit r = 1 .. n_refit: n_refine Gauss-Newton steps on sum |pi(K R^T (X - t)) - xy|^2 over the current inlier set, I_0
 *     being that of the best hypothesis, in the six unknowns (delta t, omega) with t <- t + delta t, R <- Rod(omega) R (the
 *     engine's convention).  One pass over the camera's chunks of 256 observations gives 29 sums (the 21 unique entries of
 *     J^T J, the 6 of J^T e, the cost, the count): a chunk by a fixed tree, a camera's chunks in ascending order; their
 *     combination, the 6 x 6 Cholesky, the accept rule and the pose update run on the device, one thread per camera: no host
 *     round trip per step.  A pivot <= 1e-12 x the largest diagonal entry fails the refit.  A step is taken only if it does not
 *     raise the cost; otherwise the camera keeps the previous pose and stops (the rule of mvba_triangulate).  I_r = the
 *     observations in front of the refined pose and within the threshold of it.  A refit is kept if it did not fail and
 *     |I_r| >= |I_r-1|; otherwise the loop ends with the previous result.  With n_refit = 0 the pose is the best hypothesis's.
 * R [n_cameras][9] row-major (its columns are the camera axes), t [n_cameras][3] the centre.  quality [n_cameras][2]: the RMS
 * reprojection residual over the final inliers under the pose that selected them; the smallest relative Cholesky pivot of the
 * last kept refit's last step (0 if none was kept).  n_usable, n_inliers, best [n_cameras] (best = -1 where status = 1 or 2);
 * inlier [n_obs] BYTES in the caller's observation order; hyp_count [n_cameras][n_hypotheses] (all -1 where status = 1 or 2).
 * status [n_cameras]: 0 ok; 1 fewer than 4 usable observations; 2 every hypothesis degenerate; 4 the best count is below 4 (a
 * sample guarantees 3 inliers only).  Where status != 0, R, t and quality are NaN and n_inliers is 0.
 * timings_ms [4]: sort + upload; hypotheses and scoring; refits; everything else.  Every output but R and t may be NULL.
 * Cameras are taken in tiles of 128 MiB / (196 n_hypotheses), at least 1 and at most 65535; a camera's results do not depend
 * on which other cameras are listed.  Counts are integers and every sum has a fixed order: two calls give bitwise-identical output. */
int mvba_pose_robust(const double *X, int64_t n_points, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy,
                     int64_t n_obs, int32_t n_images, const uint8_t *point_ok, const double *K, const int32_t *cameras,
                     int32_t n_cameras, double threshold, int32_t n_hypotheses, uint64_t seed, int32_t n_refine, int32_t n_refit,
                     double *R, double *t, double *quality, int64_t *n_usable, int64_t *n_inliers, int32_t *best, uint8_t *inlier,
                     int32_t *hyp_count, int32_t *status, double *timings_ms, int32_t device);
/* mvba_pose_refine: the refit of mvba_pose_robust alone -- the same kernels --, for given poses against fixed points: R
 * [n_cameras][9], t [n_cameras][3] in and out per LISTED camera; K, X, the list, point_ok and cameras as above; obs_ok [n_obs]
 * (may be NULL) != 0 marks the observations to use among the usable ones.  n_steps in 0 .. 64 Gauss-Newton steps over them; there
 * is no threshold.  status [n_cameras]: 0 ok; 1 fewer than 3 such observations; 2 the normal matrix fails the pivot rule at the
 * first step, or the input is not finite (a later failure of the rule ends the iteration at the pose reached).  A camera of
 * status != 0 keeps its input pose.  quality [n_cameras][3]: RMS reprojection residual before, after, steps taken (NaN where
 * status != 0).  n_usable [n_cameras]: the observations used.  timings_ms [3]: sort + upload, the iteration, everything else.
 * quality, n_usable, status and timings_ms may be NULL. */
int mvba_pose_refine(const double *X, int64_t n_points, const int64_t *pt_ptr, const int32_t *cam_idx, const double *xy,
                     int64_t n_obs, int32_t n_images, const uint8_t *point_ok, const uint8_t *obs_ok, const double *K,
                     const int32_t *cameras, int32_t n_cameras, int32_t n_steps, double *R, double *t, double *quality,
                     int64_t *n_usable, int32_t *status, double *timings_ms, int32_t device);
/* Host only (no GPU needed): the 4 distinct indices below n that hypothesis h of camera k draws -- mvba_ransac_sample's
 * generator with l = k and 4 draws: the first 4 of mvba_ransac_sample(seed, k, k, h, n) wherever n >= 8.  MVBA_ERR_BADARG: n
 * outside 4 .. 2^31 - 1, a negative k or h. */
int mvba_pose_sample(uint64_t seed, int32_t k, int32_t h, int64_t n, int64_t *idx4);

/* mvba_triangulate_robust: mvba_triangulate with a two-view RANSAC per point in front of it (csrc/mvba_tri_ransac.h, DESIGN.md
 * 19).  Cameras, list, dense grid (pt_ptr == NULL), units, the argument checks and the limit of 1704 cameras are
 * mvba_triangulate's; MVBA_ERR_BADARG also for a threshold that is not finite or not > 0, n_hypotheses outside 1 .. 4096 and
 * n_refit outside 0 .. 16.  Nothing is launched before the checks have passed.
 * Per point a, its deg observations numbered 0 .. deg - 1 in list order, n_pairs = deg (deg - 1) / 2:
 *   hypothesis h = 0 .. n_hypotheses - 1: two observations i < j, those of mvba_triangulate_sample(seed, a, h, deg,
 *     n_hypotheses) -- every pair once if n_pairs <= n_hypotheses, a seeded sample otherwise --; its model is the midpoint of
 *     the two viewing rays in closed form: centre c = t_k, direction d = M^-1 (x, y, 1) scaled to unit length with M = P[:, :3]
 *     inverted by its adjugate; b = c_2 - c_1, alpha = d_1 . d_2, s = (b . d_1 - alpha b . d_2) / (1 - alpha^2),
 *     u = (alpha b . d_1 - b . d_2) / (1 - alpha^2), X_h = (c_1 + s d_1 + c_2 + u d_2) / 2; degenerate if 1 - alpha^2 <= 1e-12
 *     or X_h is not finite;
 *   score: count_h = the number of the point's observations with depth P[2] . (X_h, 1) > 0 and squared reprojection distance
 *     |pi(P X_h) - xy|^2 <= threshold^2 (the test of mvba_resect_robust), an integer; -1 for a degenerate hypothesis and for a
 *     table entry h >= n_pairs of an exhaustive point; best = the largest count, the lowest h on ties;
 *   refit r = 1 .. n_refit: mvba_triangulate's fit (the DLT, then n_refine Gauss-Newton steps) on the current inlier set alone,
 *     I_0 being that of X_best; I_r = the observations in front of their camera and within the threshold of that fit.  Refit 1
 *     is kept if its status is 0 and |I_1| >= min(deg, 3); refit r >= 2 if its status is 0 and |I_r| >= |I_r-1|; otherwise the
 *     loop stops with the previous result.  With n_refit = 0, X is X_best.
 * status [n_points]: 0 ok; 1 fewer than two observations; 2 every hypothesis degenerate; 4 the best count is below
 * min(deg, 3): a point with three or more observations needs three that agree.  A point with exactly two has one
 * hypothesis, whose two observations are its own inliers whenever they lie within the threshold of the midpoint: such a point
 * CANNOT be verified, and a wrong match in it passes if the two rays happen to come close.  Where status != 0, X and quality are NaN,
 * n_inliers is 0 and none of the point's inlier bytes is set.
 * X [n_points][3].  quality [n_points][3]: mvba_triangulate's three figures over the final inliers at the returned X.
 * n_inliers, best [n_points] (best = -1 where status = 1 or 2).  inlier [n_obs] BYTES in list order: 1 for a final inlier.
 * hyp_count [n_points][n_hypotheses]: the count table.  timings_ms [4]: upload; hypotheses and scores (k_tri_score, by
 * events); refits and quality (k_tri_refit, by events); download.  Every output but X may be NULL.  A group of 16 lanes per
 * point, integer counts, no atomics: two calls give bitwise-identical output. */
int mvba_triangulate_robust(const double *K, const double *R, const double *t, int32_t n_images, int64_t n_points, const int64_t *pt_ptr,
                            const int32_t *cam_idx, const double *xy, int64_t n_obs, double threshold, int32_t n_hypotheses,
                            uint64_t seed, int32_t n_refine, int32_t n_refit, double *X, double *quality, int32_t *status,
                            int32_t *n_inliers, int32_t *best, uint8_t *inlier, int32_t *hyp_count, double *timings_ms, int32_t device);
/* Host only (no GPU needed): the two observation numbers idx2[0] < idx2[1] of hypothesis h of a point with deg observations --
 * the function the kernel runs.  n_pairs <= n_hypotheses: the h-th pair (i, j), i < j, in lexicographic order, or (-1, -1) for
 * h >= n_pairs.  Otherwise the first two draws of mvba_ransac_sample's generator with k = l = point and n = deg, sorted.
 * MVBA_ERR_BADARG: deg outside 2 .. 2^31 - 1, n_hypotheses outside 1 .. 4096, a negative point or h, h >= n_hypotheses. */
int mvba_triangulate_sample(uint64_t seed, int32_t point, int32_t h, int64_t deg, int32_t n_hypotheses, int64_t *idx2);

/* mvba_align_robust: the similarity y ~ s Q x + tau between two point sets by 3-point RANSAC -- absolute orientation: a
 * reconstruction into the frame of its control points, two maps onto each other.  src, dst [n][3]: row i of src corresponds to
 * row i of dst; ok [n] (may be NULL: every row).  A correspondence is usable if ok allows it and its six numbers are finite; the
 * usable ones are compacted in ascending order (chunks of 256, as mvba_two_view_robust compacts a pair's shared points).
 * with_scale = 0: the rigid fit, s is exactly 1.
 *   hypothesis h: the 3 indices of mvba_align_sample(seed, h, n_usable); both triples centred, Horn's symmetric 4 x 4 matrix
 *     of their cross-covariance, q = the eigenvector of its largest eigenvalue (cyclic Jacobi in registers), Q = the rotation of
 *     the unit quaternion q -- proper by construction: a reflection is never returned --, s = sum y_c . (Q x_c) / sum |x_c|^2,
 *     tau = mean(y) - s Q mean(x).  Degenerate (count -1) if either triple has |(p1 - p0) x (p2 - p0)|^2 <= 1e-12 |p1 - p0|^2
 *     |p2 - p0|^2 (collinear or coincident), the two largest eigenvalues differ by no more than 1e-12 of the largest, s is not
 *     positive or a number is not finite;
 *   count: the usable correspondences with |s Q x + tau - y|^2 <= threshold^2 (threshold in the units of dst; integer counts);
 *   best: the largest count, the lowest h on ties;
 *   refits: n_refit (0 .. 16) times at most the least-squares fit of the current inliers alone, in two passes (the centroids,
 *     then the centred moments) and the same eigen-problem on the host; the first is kept if it has 3 inliers of its own, a later
 *     one while its inlier set does not shrink (mvba_resect_robust's rule).
 * sim13 = (s, Q row-major, tau).  quality [3]: the RMS residual over the final inliers; (l1 - l2) / l1 of the two largest
 * eigenvalues of the last kept refit (0 if none); sum |x_c|^2 / count of the final inliers about their centroid.  inlier [n]
 * bytes over the input rows, hyp_count [n_hypotheses] (both may be NULL, as may quality, n_usable, n_inliers, best, status and
 * timings_ms [4]: upload, score, refit, other).  *status: 0 ok; 1 fewer than 3 usable correspondences; 2 every hypothesis
 * degenerate; 4 the best count is below 3 -- sim13 and quality NaN, inlier zero, *best -1 (status 1, 2), *n_inliers 0 then.
 * n_hypotheses 1 .. 65536, n < 2^31.  Every sum runs in an order the sizes alone fix: two calls give bitwise-identical output. */
int mvba_align_robust(int64_t n, const double *src, const double *dst, const uint8_t *ok, int32_t with_scale, double threshold,
                      int32_t n_hypotheses, uint64_t seed, int32_t n_refit, double *sim13, double *quality, int64_t *n_usable,
                      int64_t *n_inliers, int32_t *best, uint8_t *inlier, int32_t *hyp_count, int32_t *status, double *timings_ms,
                      int32_t device);
/* The plain least-squares similarity of every usable correspondence: the refit of mvba_align_robust alone.  quality [3]: the RMS
 * residual over the usable correspondences, the eigenvalue gap, sum |x_c|^2 / count.  *status: 0 ok; 1 fewer than 3 usable
 * correspondences; 2 degenerate -- src or dst on a line (the gap is at most 1e-12), coincident, or s not positive. */
int mvba_align(int64_t n, const double *src, const double *dst, const uint8_t *ok, int32_t with_scale, double *sim13, double *quality,
               int64_t *n_usable, int32_t *status, int32_t device);
/* Host only (no GPU needed): the 3 distinct indices below n that hypothesis h draws -- the first 3 of
 * mvba_ransac_sample(seed, 0, 0, h, n) wherever n >= 8.  MVBA_ERR_BADARG: n outside 3 .. 2^31 - 1, a negative h. */
int mvba_align_sample(uint64_t seed, int32_t h, int64_t n, int64_t *idx3);

/* mvba_build_tracks: feature tracks -- the observation list every entry point above takes -- from pairwise keypoint matches.
 * Keypoint j of image i is NODE kp_ptr[i] + j: kp_ptr [n_images + 1] ascends from 0, n_nodes = kp_ptr[n_images] < 2^31; ids are
 * image-major, so ascending node ids are ascending images.  kp_xy [n_nodes][2]: the keypoints' coordinates (any units; may be
 * NULL where xy is).  edges [n_edges][2]: a match is a pair of node ids.  Duplicates, either orientation, u == v and edges between
 * two keypoints of one image are all legal; edge_ok [n_edges] != 0 selects the edges to use (NULL: all of them).
 *   1. labels: the connected components of the graph, label[v] = the smallest node id of v's component.  Rounds of two
 *      launches -- every edge hooks the larger of its ends' roots under the smaller (atomicMin), then every node is pointed at
 *      its root -- until a round changes nothing; the host reads one word per round.  parent[v] <= v throughout: no kernel
 *      waits for, or retries on, another thread's write.
 *   2. sizes (integer atomics) and classes.  A component of one node is a singleton; of fewer than min_length nodes, short;
 *      of more than n_images nodes, oversize -- two of its nodes share an image whatever they are, and it is dropped without
 *      being laid out (a few wrong matches chain thousands of tracks into one); the first of these that holds decides.  Every
 *      other component is a candidate.
 *   3. the candidates laid out (an exclusive scan of their sizes in ascending label order), each sorted by node id.  A
 *      candidate with two nodes in one image is CONFLICTING and is dropped whole: it is neither pruned nor split.
 *   4. the surviving tracks numbered in ascending order of their smallest node id:
 * pt_ptr [n_tracks + 1], cam_idx [n_obs] (ascending within a track), obs_node [n_obs] (the node of every observation),
 * xy [n_obs][2] = kp_xy[obs_node] (a copy made on the device; NULL: not wanted), node_track [n_nodes]: >= 0 the node's track,
 * -1 unmatched (a singleton), -2 its component is shorter than min_length, -3 its component conflicts or is oversize.
 * The caller sizes cam_idx, obs_node, xy and node_track by n_nodes, and pt_ptr by n_nodes / 2 + 1.
 * counts [10]: tracks, observations, components of two nodes or more, short components, conflicting components, their nodes,
 * oversize components, their nodes, singletons, rounds (the last, unchanging one included; 0 without edges).
 * timings_ms [4] (may be NULL): upload (with the checks), labels, layout (steps 2 to 4), download and everything else.
 * No floating-point arithmetic anywhere: the outputs are a function of the SET of used edges -- permuted, turned round or
 * duplicated edges, and a second call, give bitwise equal arrays.
 * MVBA_ERR_BADARG, before any device work and with the number in the message: a null kp_ptr, pt_ptr, cam_idx, obs_node,
 * node_track or counts (named, with its position), kp_xy NULL with an xy, edges NULL with n_edges > 0; n_edges < 0;
 * min_length < 2; n_images < 1; kp_ptr not ascending from 0; n_nodes >= 2^31; a node id outside 0 .. n_nodes - 1 (the edge
 * and the id are named). */
int mvba_build_tracks(int32_t n_images, const int64_t *kp_ptr, const double *kp_xy, const int32_t *edges, int64_t n_edges,
                      const uint8_t *edge_ok, int32_t min_length, int64_t *pt_ptr, int32_t *cam_idx, int32_t *obs_node, double *xy,
                      int32_t *node_track, int64_t *counts, double *timings_ms, int32_t device);

/* mvba_match_descriptors: the matches that mvba_build_tracks takes, from uint8 descriptors, by brute force.  Keypoint j of image
 * i is node kp_ptr[i] + j, as above; its descriptor is row kp_ptr[i] + j of desc [n_nodes][dim], dim unsigned bytes (SIFT as
 * COLMAP and VisualSFM store it: dim = 128).  pairs [n_pairs][2]: for the pair (k, l), k is the QUERY image and l the CANDIDATE
 * image.  For every keypoint a of k, over the keypoints b of l:
 *   d2(a, b) = sum (desc_k[a] - desc_l[b])^2, an exact integer (below 2^25 at dim = 512; computed on the i8 matrix cores as
 *     |a'|^2 + |b'|^2 - 2 a'.b' with every byte shifted by 128, which changes no distance);
 *   best(a): the b with the smallest (d2, b) -- a tie in distance goes to the smaller index;
 *   second(a): the smallest d2 over b != best(a); it may equal the best distance;
 *   with n_l == 0 there is no best, with n_l == 1 no second (reported as -1).
 * a is matched to best(a) unless, the first that holds (each is counted):
 *   1. no candidate: n_l == 0;
 *   2. far: max_dist2 >= 0 and d2_best > max_dist2;
 *   3. ambiguous: ratio > 0 and there is no second, or NOT (double) d2_best < r2 * (double) d2_second, where r2 = ratio * ratio is
 *      rounded once, in double, on the host; the device makes one double multiply and one compare (no addition: nothing to
 *      contract).  A keypoint with a single candidate passes no ratio test;
 *   4. not mutual: mutual != 0 and best(b), the nearest keypoint of image k to b = best(a) by the same rule with the roles
 *      swapped (ties to the smaller index), is not a.  The reverse direction takes no ratio or distance test.
 * ratio in (0, 1], or 0 for no ratio test; max_dist2 < 0 for no distance test.  Pairs are answered in the order given and each
 * whatever the rest of the list: a duplicated pair is answered twice, a pair (l, k) with l > k is answered as given.
 * Q = the sum of the query images' keypoint counts over the pairs.  match_ptr [n_pairs + 1]; kp_pairs [Q][2] and dist2 [Q] (sized
 * by the caller; match_ptr[n_pairs] rows are written): the matches of pair p are rows match_ptr[p] .. match_ptr[p + 1] - 1,
 * [a, b] local to their images, ascending a, with their d2.  nn_best, nn_dist2, nn_second2 [Q] (each may be NULL): in query
 * order per pair, every query's best index (-1: none), best d2 (-1: none) and second d2 (-1: none), before any test.
 * counts [6]: matches, queries (Q), no candidate, far, ambiguous, not mutual; the matches and the four rules' counts add up
 * to Q.  timings_ms [4] (may be NULL): checks and upload; distances; tests and compaction; download and the rest.
 * All descriptors go to the device once per call; the pairs are worked through in chunks of about 4 M query rows, so the
 * per-query temporaries stay bounded.  One workgroup owns 128 queries of one direction of one pair and sweeps all candidates:
 * many pairs fill the device, one small pair does not.  Integers only (but for the compare of rule 3) and no atomics: the outputs
 * are a function of the input alone, bitwise equal from call to call.
 * MVBA_ERR_BADARG, before any device work and with the number in the message: a null kp_ptr, match_ptr, kp_pairs, dist2 or
 * counts (named, with its position); desc NULL with keypoints present; pairs NULL with n_pairs > 0; n_pairs < 0; n_images < 1;
 * kp_ptr not ascending from 0; n_nodes >= 2^31; Q >= 2^31; dim not a multiple of 16 in 16 .. 512; ratio outside [0, 1] or NaN;
 * an image index out of range (the pair and the index are named); a pair of an image with itself.  With n_pairs == 0, or every
 * query image empty, MVBA_OK with a complete answer (match_ptr all 0, counts 0) and no device work. */
int mvba_match_descriptors(int32_t n_images, const int64_t *kp_ptr, const uint8_t *desc, int32_t dim, const int32_t *pairs,
                           int32_t n_pairs, double ratio, int32_t mutual, int64_t max_dist2, int64_t *match_ptr, int32_t *kp_pairs,
                           int32_t *dist2, int32_t *nn_best, int32_t *nn_dist2, int32_t *nn_second2, int64_t *counts,
                           double *timings_ms, int32_t device);

/* Host-only check of the per-observation math the kernels use (no GPU needed):
 * cam15 = f,u,v,t[3],R[9]; out = e[2], JX[6], JC[18].                          */
int mvba_host_obs_math(const double *X3, const double *cam15, const double *xy2, double f0,
                       double *out26);

/* ---- factorization (ref lib/factorization.py:5-15) ---------------------------
 * Wt: the measurement matrix as its callers hold it, row-major [n_rows][n_cols]
 * with n_rows = points (tall) and n_cols = 2m or 3m; the reference's W is Wt^T
 * (perspective_camera_calibration.py:533, affine_camera_calibration.py:236).
 * dtype: 0 = float32, 1 = float64 (outputs have the input dtype, ref quirk B.10).
 * center != 0: subtract the column means of Wt first (= the row means of W the
 * affine callers remove, affine_camera_calibration.py:224-240); means [n_cols]
 * receives them (may be NULL).
 * Outputs: M [n_cols][n_rank] (= U[:, :r]), sigma [n_cols] (singular values,
 * descending), S [n_rank][n_rows] (= diag(sigma[:r]) Vt[:r] = M^T W).  Thin: Vt is
 * never formed.  Sign convention: the largest-magnitude component of every column
 * of M is positive (LAPACK's signs are not a rule one can restate).
 * Two routes.  n_cols <= 64, or n_rank > 16 with n_cols <= 256: Gram matrix + Jacobi, n_rank any 1 .. n_cols, sigma = every
 * singular value.  Otherwise (65 .. 12288 columns = three rows per image at the engine's 4096 cameras, n_rank <= 16; MVBA_ERR_BADARG
 * beyond either): block power iteration with Rayleigh-Ritz on W^T W applied implicitly, 32 vectors wide, two passes over W per
 * iteration, no n_cols x n_cols matrix; sigma[0..31] = the block's Ritz values (the leading n_rank converged), sigma[32..] = NaN;
 * MVBA_ERR_SINGULAR ("SVD did not converge", LAPACK's own failure) after 2000 iterations.
 * Accuracy: float32 data -> one Gram pass accumulated in fp64 (nothing is lost: eps32 >> eps64 *
 * cond^2); float64 data -> a second, preconditioned pass so that small singular values are good to
 * ~eps64 * sigma_1 like LAPACK's gesdd, not to sqrt(eps64) * sigma_1 (see csrc/mvsvd.hip).
 * timings_ms (may be NULL) [6]: H2D, means + Gram, Jacobi, projection (device ms), sweeps,
 * refinement pass (0 for float32).  Block route: H2D, means, the iteration, S out of the last product, iterations, final pass. */
int mvsvd_factorize(const void *Wt, int64_t n_rows, int32_t n_cols, int32_t dtype, int32_t n_rank,
                    int32_t center, void *M, void *sigma, void *S, void *means, double *timings_ms,
                    int32_t device);

/* Workspace form for repeated factorizations (the projective-depth loops call the SVD 50-200
 * times, ref perspective_camera_calibration.py:61-144, :147-235): create once (device buffers
 * for up to max_rows x n_cols, stream, events), load a matrix (the only host-to-device copy),
 * run any number of factorizations on the resident matrix (different n_rank / center), destroy. */
typedef struct mvsvd_handle mvsvd_handle;
int mvsvd_create(int64_t max_rows, int32_t n_cols, int32_t dtype, int32_t device, mvsvd_handle **out);
int mvsvd_load(mvsvd_handle *h, const void *Wt, int64_t n_rows);
/* The same matrix put together on the device from the images' own arrays -- what the reference's callers hold
 * (ref lib/affine_camera_calibration.py:224-240: W = np.hstack(data_list).T; the hstack alone is 0.3 s of strided host writes at
 * 5 M points x 12 images, twenty times the upload + factorisation): xy[k] = image k's coordinates [n_rows][2], float32
 * (src_dtype 0) or float64 (1), converted to the workspace's dtype; W^T[i][2k .. 2k+1] = xy[k][i]; n_cols must be 2 n_images. */
int mvsvd_load_images(mvsvd_handle *h, const void *const *xy, int32_t n_images, int64_t n_rows, int32_t src_dtype);
int mvsvd_run(mvsvd_handle *h, int32_t n_rank, int32_t center, void *M, void *sigma, void *S, void *means,
              double *timings_ms);

/* The projective-depth loops (ref perspective_camera_calibration.py:61-144, :147-235) factorise, 50-200 times,
 * the SAME homogeneous observations X re-weighted by the current depths: W[a][g*group + c] = X[a][g*group + c] *
 * z[a][g] * s with s = 1 / |row a of X o z| (norm 1: every row -- point -- to unit length, ref :86-87), s = 1 / sum of
 * the group's (X o z)^2 over all rows (norm 2: every column group -- image -- divided by its squared Frobenius
 * norm, ref :170-172) or s = 1 (norm 0).  mvsvd_load_base uploads X (n_rows x n_cols, the workspace's dtype) once;
 * every mvsvd_run_scaled uploads only z (n_rows x n_cols / group), forms W on the device and runs the factorisation
 * (no centring).  timings_ms[0] is then the upload of z.  z == NULL: the depths a device depth loop (below) left in the workspace,
 * same grouping -- nothing is uploaded: the final factorisation of perspective_self_calibration (ref :531-533) without W on the host. */
int mvsvd_load_base(mvsvd_handle *h, const void *X, int64_t n_rows);
/* The same base assembled on the device from the images' own arrays (ref lib/perspective_camera_calibration.py:34-40,
 * _create_data_matrix: 0.11 s of strided host writes at 1 M points x 12 images, and a third more bytes over PCIe):
 * xy[k] = image k's pixel coordinates [n_rows][2] (doubles), base[i][3k .. 3k+2] = (x / f0, y / f0, 1) in the workspace's
 * dtype; n_cols of the workspace must be 3 n_images. */
int mvsvd_load_base_images(mvsvd_handle *h, const double *const *xy, int32_t n_images, int64_t n_rows, double f0);
int mvsvd_run_scaled(mvsvd_handle *h, const void *z, int32_t group, int32_t norm, int32_t n_rank, void *M, void *sigma, void *S,
                     double *timings_ms);

/* The depth UPDATE of those loops on the device too (ref perspective_camera_calibration.py:93-129 primary, :182-224
 * dual): the depths z live in the workspace, and one mvsvd_depth_step is one whole iteration of the reference's loop --
 * re-weight the resident X by z and normalise (norm = method), rank-4 factorisation, then per point (method 1, primary)
 * the dominant eigenvector of the m x m matrix of :99-107 from its 4 x 4 companion, or per image (method 2, dual) that
 * of the N x N matrix of :188-205 from its 12 x 12 companion (O(N) memory), the sign rules of :121 / :217,
 * z <- xi / |x| (:124 / :220) and the reprojection error of :43-58 into *E.  Per iteration 8 bytes cross PCIe.
 * mvsvd_depth_begin (after mvsvd_load_base; group must be 3: homogeneous image coordinates, n_cols = 3 m) sets
 * z = 1 (:75 / :160); mvsvd_depth_read downloads the depths [n_rows][m] (the workspace's dtype), once, at the end.
 * A new base (mvsvd_load_base / _images) ends the loop: step, read and run_scaled(z = NULL) give MVBA_ERR_STATE until depth_begin.
 * timings_ms (may be NULL) [6] as in mvsvd_run, except slot 0: device ms of the depth-update kernels.
 * MVBA_ERR_SINGULAR: the re-weighted matrix has rank < 4. */
int mvsvd_depth_begin(mvsvd_handle *h, int32_t group);
int mvsvd_depth_step(mvsvd_handle *h, int32_t method, double f0, double *E, double *timings_ms);
int mvsvd_depth_read(mvsvd_handle *h, void *z);
void mvsvd_destroy(mvsvd_handle *h);

#ifdef __cplusplus
}
#endif
#endif /* MVBA_H */
