/*
 * bcqp.h — C ABI of the MI355X-native box-constrained dual-QP hot path (libbcqp_hip.so).
 *
 * The reference (dmeoli/optiml) is pure Python/NumPy and has NO FFI; its "operator API" for this
 * path is the Python class surface.  Each entry point below replaces the NumPy/SciPy arithmetic of
 * one reference site (paths relative to the reference checkout); the Python classes in
 * optiml_amd/ keep the reference's names and ctor arguments and bind these symbols with ctypes
 * (see INTEGRATION.md for the binding a reference maintainer would add).
 *
 *   min 1/2 x'Qx + q'x   s.t.  lb <= x <= ub
 *
 * Conventions
 *   - every function returns an int: 0 = ok, <0 = error class (BQ_ERR_*); the message of the last
 *     error on the calling thread is returned by bq_last_error().
 *   - host buffers are BORROWED for the duration of the call, never retained.
 *   - device memory is owned by the opaque handles and released by the *_destroy functions.
 *   - a bq_ctx is not thread-safe; every call returns after its HIP stream has been synchronised.
 *   - all host-visible vectors are fp64.  `storage` selects the dtype of the resident Hessian /
 *     Gram panel only (fp32 storage still accumulates in fp64).
 *   - multi-GPU: one process per GPU; all n-vectors are replicated and each product Q*v is completed
 *     by ONE collective (RCCL over xGMI, or a caller-supplied exchange callback): kernel-built
 *     symmetric panels are split into tile rows with equal shares of the lower triangle
 *     (bq_sym_row_block: runs of 8 canonical segments) and end in an all-gather of the per-segment
 *     partial vectors, which every rank adds in segment order — bit-identical iterates for 1/2/4/8
 *     ranks (BQ_SYM_EXCHANGE=allreduce: one all-reduce(sum) instead); a dense Q that equals its transpose
 *     exactly is stored and split the same way; any other dense Q is split into equal row blocks
 *     (bq_row_block) and ends in an all-gather.  Solvers that factorise the Hessian (InteriorPoint,
 *     ActiveSet) and SMO need a single-rank context.
 */
#ifndef BCQP_H
#define BCQP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BQ_OK 0
#define BQ_ERR_HIP (-1)       /* a HIP runtime call failed */
#define BQ_ERR_RCCL (-2)      /* RCCL missing or a collective failed */
#define BQ_ERR_NOT_PD (-3)    /* Cholesky met a non-positive pivot (scipy: LinAlgError) */
#define BQ_ERR_NONFINITE (-4) /* inf/nan where the reference would raise (e.g. IP with ub=inf) */
#define BQ_ERR_BADARG (-5)
#define BQ_ERR_NOMEM (-6)

/* 2 (round 6): bq_ctx_probe_stall takes behind_collective, bq_problem_create_dense takes layout flags, bq_problem_layout,
 * bq_ctx_release_held_memory and the state snapshot were added: a consumer built against version 1 must be rebuilt */
/* 3: the batched one-vs-rest solver (bq_msolver_*) and bq_problem_gram_matmat were added */
/* (still 3: bq_msolver_create_boxes and bq_problem_gram_matmat_wide were added; nothing existing changed) */
/* (still 3: bq_msolver_create_pairs, bq_problem_gram_matmat_pairs, bq_pairs_slab_bytes and bq_pairs_work_list were added) */
/* (still 3: the structure flag BQ_PLAIN_PANEL was added) */
/* (still 3: bq_msolver_create_svr was added) */
/* (still 3: bq_msolver_create_svr_boxes and bq_msolver_svr_heldout were added; nothing existing changed) */
/* (still 3: bq_msolver_create_al was added; nothing existing changed) */
/* (still 3: bq_platt_fit and bq_msolver_svc_heldout were added; nothing existing changed) */
/* (still 3: bq_problem_hessian_image and the test entry bq_problem_last_product were added; nothing existing changed) */
/* (still 3: bq_msolver_pairs_heldout, bq_pairwise_coupling and bq_decision_coupled were added; nothing existing changed) */
/* (still 3: bq_msolver_create_simplex, bq_msolver_simplex_offsets and bq_simplex_project were added; nothing existing changed) */
/* (still 3: bq_msolver_create_simplex2 and bq_msolver_simplex2_offsets were added; nothing existing changed) */
/* (still 3: bq_msolver_create_simplex2_pairs was added; nothing existing changed) */
/* (still 3: bq_msolver_simplex2_heldout was added; nothing existing changed) */
/* (still 3: bq_ovo_vote and bq_msolver_pairs_vote_heldout were added; nothing existing changed) */
/* (still 3: bq_msmo_create / _run / _get / _destroy were added; nothing existing changed) */
/* (still 3: bq_msmo_vote_heldout was added; nothing existing changed) */
/* (still 3: bq_msmo_svr_heldout and bq_msmo_svc_heldout were added; nothing existing changed) */
/* (still 3: bq_rsmo_create / _run / _get / _rows / _destroy were added; nothing existing changed) */
/* (still 3: bq_rsmo_create_general and BQ_RSMO_NU_SCALARS were added; nothing existing changed) */
#define BQ_ABI_VERSION 3

typedef struct bq_ctx bq_ctx;
typedef struct bq_problem bq_problem;
typedef struct bq_solver bq_solver;
typedef struct bq_msolver bq_msolver;

/* panel storage: fp64, fp32 (fp64 accumulation), or none at all — BQ_STREAM recomputes the Gram tiles on the MFMA inside
 * every product (kernel problems with an inner-product kernel; PG / FW / augmented-Lagrangian solvers only): the
 * fallback for n^2 s > HBM */
enum { BQ_F64 = 0, BQ_F32 = 1, BQ_STREAM = 2 };
/* linear, poly, rbf: kernels.py:40-129 (the named configs); sigmoid, laplacian: kernels.py:132-201 */
enum { BQ_KERNEL_LINEAR = 0, BQ_KERNEL_POLY = 1, BQ_KERNEL_RBF = 2, BQ_KERNEL_SIGMOID = 3, BQ_KERNEL_LAPLACIAN = 4 };
enum { BQ_PLAIN = 0, BQ_SVC = 1, BQ_SVR = 2 };                       /* Hessian structure */
/* OR-ed into the structure: leave out the rank-one term yy' / ee' of the regularised intercept, i.e. the
 * reg_intercept=False duals Q = K*yy' and Q = [[K,-K],[-K,K]] (svm/_base.py:552-559, 1096-1099).  Products only:
 * InteriorPoint / ActiveSet refuse such a problem (the reference has no box solver for it either, :621-624). */
#define BQ_NO_RANK_ONE 16
/* OR-ed into the structure: keep the WHOLE n x n Gram panel (row blocks, pitch round_up(n, 1024)) instead of the packed
 * lower-triangular tile rows: twice the memory and twice the bytes per product, but every row is contiguous and K keeps
 * the reference's own (not exactly symmetric) rounding of the RBF distances.  An option, not a default: measured on SMO
 * (single-row gathers) it changes nothing, n=100k fit 0.93 s either way — the sweeps are bound by one CU's gather rate.
 * The factorising solvers and bq_problem_x_star read the upper triangle of such a panel (as of dense row blocks, below). */
#define BQ_FULL_PANEL 32
/* OR-ed into the structure: choose WHERE the resident panel lives.  The rate at which the panel product streams a panel is a
 * stable property of the physical region the allocation landed in (five panels of one n = 100 000 problem held at once ran 6.04 -
 * 6.50 ms per product, each reproducible to 0.005 ms; NOT of its base address, nor of the contiguity the API can ask for:
 * profiles/r04/placement_*.txt): with this flag the product kernel is timed on the freshly allocated (still empty) panel and, if
 * it streams below ~6.5 TB/s, further allocations are tried while they fit a time budget (BQ_PLACE_BUDGET_MS, default 200 ms; at
 * most 3; a candidate is priced at what the first allocation cost; bq_ctx_set_placement_budget lets the budget grow with the work
 * the caller expects) and the fastest is kept (the others are held until the solve is over: bq_ctx_set_placement_budget; a candidate is only tried while a
 * tenth of the device stays free beside it).  For the product-bound solvers (PG, FW, ActiveSetCG, the
 * augmented-Lagrangian rules), whose every iteration streams the panel — SVC / SVR.fit set it for those; pointless for
 * InteriorPoint / ActiveSet / SMO.  Per rank, before the first collective. */
#define BQ_PLACE_PANEL 64
/* OR-ed into the structure: keep the fp64 panel at 8 bytes per element even where the lossless 7-byte layout applies (see
 * bq_problem_layout).  For SMO, whose sweeps gather single elements: there one element costs three loads instead of one
 * (measured at n = 100 000: SVC.fit(optimizer='smo') 0.39 s plain, 0.50 s compact). */
#define BQ_PLAIN_PANEL 128
enum { BQ_PG = 0, BQ_FW = 1, BQ_AS = 2, BQ_IP = 3,                   /* solver kind */
       /* ActiveSet (active_set.py:82-237, same outer logic) whose restricted systems Q[A,A] xs = rhs are solved by
        * conjugate gradients on the masked panel product instead of a dense Cholesky factor: no n_A x n_A copy, so it
        * also runs on sharded (multi-rank), fp32-stored and streamed panels — SURVEY 7's plan for config 5.  The inner
        * iteration stops at |r| <= rtol (|(Q x)_A| + |q_A|); a direction of non-positive curvature is BQ_ERR_NOT_PD. */
       BQ_AS_CG = 5 };
enum { BQ_STATUS_UNKNOWN = 0, BQ_STATUS_OPTIMAL = 1, BQ_STATUS_STOPPED = 2 };
/* BQ_GET_X / BQ_GET_G: the point (and gradient) the LAST ITERATION RECORD was evaluated at — what the
 * reference's callback sees at the top of that iteration.  BQ_GET_X_NOW / BQ_GET_G_NOW: the current iterate
 * (differs only for ActiveSet, whose loop body moves x after the record: active_set.py:156-160, 208). */
enum { BQ_GET_X = 0, BQ_GET_G = 1, BQ_GET_LP = 2, BQ_GET_LM = 3, BQ_GET_D = 4,
       BQ_GET_MASK_L = 5, BQ_GET_MASK_U = 6, BQ_GET_X_NOW = 7, BQ_GET_G_NOW = 8,
       BQ_GET_DUAL = 9 /* augmented Lagrangian: [mu (if a_eq); lambda_lb (if lb); lambda_ub (if ub)] */ };

/* One row per evaluation at the top of a solver iteration (what the reference's callback/verbose
 * line sees).  r1/r2/r3 by solver:  PG: |proj grad|_2, step t, max_t;  FW: best lower bound, gap,
 * step a;  IP: dual value p, gap, step;  AS: |L|+|U|, event (0 step / 1 release-L / 2 release-U /
 * 3 optimal) , index or count. */
typedef struct bq_iter_stat {
    int64_t iter;
    double f;
    double r1, r2, r3;
} bq_iter_stat;

/* Exchange callback for multi-process runs without RCCL (tests; hosts without xGMI).  Return 0 on success.
 *   op 0 (gather): on entry buf holds this rank's rows [row_begin,row_end) of an n-vector; on return the whole
 *                  vector must be filled with every rank's rows   (row-block panels; the segment partials of the
 *                  symmetric tile panels: n = world * chunk, equal chunks)
 *   op 1 (sum):    on return buf[0:n) must hold the element-wise sum over ranks   (BQ_SYM_EXCHANGE=allreduce) */
typedef int (*bq_exchange_fn)(void *user, double *buf, int64_t n, int64_t row_begin, int64_t row_end, int op);

int bq_abi_version(void);
const char *bq_last_error(void);

/* ---- context -------------------------------------------------------------------------------- */
int bq_device_count(int *count);
int bq_ctx_create(int device, bq_ctx **out);
/* uid: 128-byte RCCL unique id, created on rank 0 by bq_comm_unique_id and broadcast by the caller */
int bq_comm_unique_id(void *uid128);
int bq_ctx_create_rccl(int device, int rank, int world, const void *uid128, bq_ctx **out);
/* where the time of RCCL's start-up went in this process so far: "dlopen(librccl.so) 0.41 s; dlsym x8 0.00 s; ncclGetUniqueId ...;
 * ncclCommInitRank ...; ncclCommCount ..." (empty when RCCL was never loaded).  A stage still running after 5 s also says so on
 * stderr every 5 s while it runs; NCCL_DEBUG=INFO prints every stage as it ends. */
int bq_comm_init_report(char *buf, size_t cap);
int bq_ctx_create_exchange(int device, int rank, int world, bq_exchange_fn fn, void *user, bq_ctx **out);
/* ONE rank's share of a `world`-way partition with no transport behind it: panels, segments and every kernel of the
 * per-rank iteration are exactly those of rank `rank` of `world`, every collective is a no-op — so products hold this rank's
 * contributions only.  For timing and inspecting a share on a single GPU (bench.py --emulate-shares); never a solver. */
int bq_ctx_create_share(int device, int rank, int world, bq_ctx **out);
int bq_ctx_destroy(bq_ctx *ctx);
int bq_ctx_info(const bq_ctx *ctx, int *device, int *rank, int *world, char *name, size_t name_cap);
/* the exchange behind a multi-rank context: kind 0 none / 1 RCCL / 2 callback / 3 share (bq_ctx_create_share); comm_ranks = ncclCommCount of the live
 * communicator (0 without RCCL); sym_allreduce = 1 when symmetric products end in an all-reduce (BQ_SYM_EXCHANGE=allreduce)
 * instead of the default all-gather of segment partials summed in a fixed order (bit-identical for any rank count) */
int bq_ctx_comm_info(const bq_ctx *ctx, int *kind, int *comm_ranks, int *sym_allreduce);
/* choose the closing collective of symmetric products (before the first problem is created): 0 = all-gather of segment
 * partials + ordered sum (default), 1 = all-reduce(sum) */
int bq_ctx_set_sym_allreduce(bq_ctx *ctx, int on);
/* HIP-event timing of the dominant kernels (on the stream they run on).  which: 0 = Q*v panel
 * product, 1 = Gram build, 2 = Cholesky factorisation, 3 = row-block exchange, 4 = the sample-sharded part of ActiveSetCG's
 * preconditioner (the implicit order-2 remainder: what divides by the rank count; bench.py's prediction for config 5 over 8). */
int bq_ctx_profile(bq_ctx *ctx, int enable);
int bq_ctx_profile_read(bq_ctx *ctx, int which, double *total_ms, int64_t *launches, int reset);
/* measured HBM ceilings of this GPU on a scratch buffer of `bytes`: a read-only streaming sweep and a
 * device-to-device copy (read + written bytes), in GB/s — the yardstick beside the nominal 8 TB/s */
int bq_ctx_probe_bandwidth(bq_ctx *ctx, int64_t bytes, int reps, double *read_gbs, double *copy_gbs);
/* measured fp64 matrix-core ceiling of this GPU: back-to-back v_mfma_f64_16x16x4_f64 on register operands for about `seconds`
 * (first half warm-up: the clock settles under the load), in TFLOP/s — the yardstick beside the nominal 78.6 TFLOP/s for
 * the roofline fraction of the Cholesky (SURVEY 8d asks for nominal-peak and measured fractions) */
int bq_ctx_probe_mfma_f64(bq_ctx *ctx, double seconds, double *tflops);
/* measured cost of this context's closing collective of a product (ONE collective per Q*v), on the context's stream
 * with HIP events around every call: kind 0 = the in-place all-gather of `count` doubles per rank (buffer world * count), kind 1
 * = the in-place all-reduce(sum) of `count` doubles.  `reps` calls after 3 warm-up calls; mean and minimum in microseconds.
 * On a ONE-rank RCCL communicator this is the launch + local-copy floor of the collective (a lower bound of what N > 1 ranks pay
 * over xGMI, nothing more); on N > 1 ranks every rank must call it with the same arguments. */
int bq_ctx_probe_exchange(bq_ctx *ctx, int kind, int64_t count, int reps, double *mean_us, double *min_us);
/* Bound the collectives of an RCCL context in time (0: no bound, the default; also BQ_COLLECTIVE_TIMEOUT_S through the Python
 * Context).  RCCL itself never gives up on a collective whose peer does not arrive (a rank-local error, a dead process): with a
 * timeout a watchdog thread aborts the communicator (ncclCommAbort) once the host has waited for longer on a stream that holds a
 * collective enqueued since it was last seen empty; the call in progress returns BQ_ERR_RCCL and the context is unusable afterwards.
 * A wait with only this rank's own kernels ahead of it is never cut short.  The callback transport is bounded by the caller's own
 * communicator (and on every context without an RCCL communicator the setting is accepted and does nothing).  Set it from the thread
 * that owns the context, while no call is in progress. */
int bq_ctx_set_collective_timeout(bq_ctx *ctx, double seconds);
/* occupy the compute stream for `milliseconds` (one lane spinning on the wall clock; it ends by itself) and wait for it through
 * the library's bounded wait.  behind_collective != 0: the context's collective (an all-reduce of one double) is enqueued BEHIND the
 * occupation first — what a peer that arrives `milliseconds` late looks like from this rank: the end-to-end test of the watchdog on
 * one GPU (BQ_ERR_RCCL when it fired).  behind_collective == 0: nothing but this rank's own work is ahead of the wait, which the
 * watchdog must leave alone however long it lasts (a factorisation, a preconditioner rebuild). */
int bq_ctx_probe_stall(bq_ctx *ctx, double milliseconds, int behind_collective);
/* the last-workgroup hand-off that closes every O(n) kernel of the single-problem solvers (csrc/bq_reduce.h), checked directly:
 * `rounds` launches of `blocks` workgroups back to back on the stream; in each, every workgroup stores one partial that depends on
 * (workgroup, round) and takes the ticket, and the workgroup that arrives last compares EVERY partial with its expected word.
 * uneven != 0: a workgroup-dependent amount of arithmetic first.  bad_words: mismatches over all rounds (0 is the only correct
 * answer); ticket_after: the ticket once the stream has drained (0: the last workgroup of every round set it back).  No workgroup
 * waits for another, so the call ends whatever it finds. */
int bq_ctx_probe_last_block(bq_ctx *ctx, int blocks, int rounds, int uneven, int64_t *bad_words, int *ticket_after);
/* row block [begin,end) of an n-row panel owned by `rank` out of `world` (pure arithmetic): equal 128-aligned
 * blocks for dense panels; bq_sym_row_block: the balanced triangular partition (256-aligned) of the symmetric
 * kernel panels, whose ranks stream only the tiles on/below the diagonal */
int bq_row_block(int64_t n, int rank, int world, int64_t *begin, int64_t *end);
int bq_sym_row_block(int64_t n, int rank, int world, int64_t *begin, int64_t *end);

/* ---- the quadratic ("Quadratic", optiml/opti/_base.py:228-300) ------------------------------- */
/* dense Q (n x n row-major fp64) and q: replaces the host copy at optiml/opti/_base.py:243.
 * Layout of the resident copy (bq_problem_layout tells which one was taken):
 *   - Q == Q' exactly (every pair of elements compared as stored, on the device, while the rows are uploaded; on a multi-rank
 *     context the ranks agree with one all-reduce, so the call is collective there): the packed lower-triangular 256-tile rows of
 *     the kernel-built panels — half the HBM and half the bytes per product (40 GB and ~6 ms instead of 80 GB and ~12 ms at
 *     n = 100 000), sharded by the canonical segments, bit-identical products for any rank count;
 *   - any other Q (the reference never checks symmetry, opti/_base.py:249-256, and computes `Q @ x`): whole row blocks.
 * OR-ed into `storage`:  BQ_DENSE_ROWS   row blocks whatever Q is (the layout of rounds 1-5; what a comparison needs);
 *                        BQ_DENSE_LOWER  the caller vouches for symmetry: only the lower triangle of the host matrix is read
 *                                        (LAPACK's uplo = 'L'), nothing is compared, half the PCIe traffic;
 *                        BQ_PLACE_PANEL  as for kernel problems (packed layout only).
 * Which triangle a FACTORISATION reads (InteriorPoint, ActiveSet, bq_problem_x_star assemble a symmetric H from the resident
 * copy, one triangle mirrored, as LAPACK's potrf does): of row blocks the UPPER one, H[i][j] = Q[min(i,j)][max(i,j)] — scipy's
 * cho_factor default (lower=False), i.e. what the reference's cho_factor(Q), cho_factor(Q[A,:][:,A]) and cho_factor(H) read
 * (opti/_base.py:263, active_set.py:141, interior_point.py:235); of the packed layout the lower one, which for a Q == Q' is the
 * same matrix and for BQ_DENSE_LOWER is all that was ever read.  Products, f and g always apply Q as given (`Q @ x`).
 * ActiveSet's kept factor and its product-free f of ratio steps rest on H == Q.  On row blocks they stay on while the resident
 * copy is symmetric up to rounding, max |Q_ij - Q_ji| <= 64 ulps of max |Q_ij| (measured once per problem: a Q assembled in
 * floating point); on a Q that is not symmetric every iteration factorises Q[A,A] afresh and forms f by a product, as the
 * reference does (BQ_COUNT_REUSED and BQ_COUNT_NO_PRODUCT stay 0). */
#define BQ_DENSE_ROWS 256
#define BQ_DENSE_LOWER 512
int bq_problem_create_dense(bq_ctx *ctx, int64_t n, const double *Q, const double *q, int storage,
                            bq_problem **out);
/* kernel-structured Hessian built on the device from X (n x d row-major fp64):
 *   K = kernel(X, X)                        optiml/ml/svm/kernels.py:49-51 / 91-95 / 125-129
 *   BQ_SVC: Q = K*yy' + yy' (+ diag_add*I), dual dim n     optiml/ml/svm/_base.py:552-555, 628, 729-730
 *   BQ_SVR: Q = [[K,-K],[-K,K]] + ee', dual dim 2n         optiml/ml/svm/_base.py:1096-1099, 1178
 *   BQ_PLAIN: Q = K (+ diag_add*I)
 * gamma must already be resolved ('scale'/'auto' are host-side scalars of X).  q has the dual dim. */
int bq_problem_create_kernel(bq_ctx *ctx, int structure, int64_t n, int64_t d, const double *X,
                             const double *y, int kernel, double gamma, double coef0, int degree,
                             double diag_add, const double *q, int storage, bq_problem **out);
/* destroy: device memory goes back to the driver, except that a context keeps the ONE most recently released panel of
 * >= 1 GB for the next problem of about that size (a large hipMalloc right after a large hipFree costs seconds on this
 * platform); it is released when an allocation fails and with the context. */
int bq_problem_destroy(bq_problem *p);
int bq_problem_dims(const bq_problem *p, int64_t *n_dual, int64_t *n_rows, int64_t *row_begin,
                    int64_t *row_end);
/* how the Hessian is resident on this rank: *packed = 1 for the packed lower tile rows (kernel-built panels; a dense Q == Q'),
 * 0 for row blocks; *streamed = 1 for BQ_STREAM (no panel); *panel_bytes = the size of this rank's panel allocation.  An RBF
 * panel in BQ_F64 whose every entry lies in [2^-14, 1] (exp(-gamma 4 max |x_i|^2) >= 2^-14) is kept losslessly in 7 bytes per
 * element instead of 8 (its top byte is known): its panel_bytes are 7/8 of the fp64 size; values and products do not change. */
int bq_problem_layout(const bq_problem *p, int *packed, int *streamed, int64_t *panel_bytes);
/* out = Q v (dual dim; every rank gets the full vector)       optiml/opti/_base.py:291 (minus q) */
int bq_problem_matvec(bq_problem *p, const double *v, double *out);
/* f = 1/2 x'Qx + q'x and (optionally, g != NULL) g = Qx + q   optiml/opti/_base.py:282, 291 */
int bq_problem_eval(bq_problem *p, const double *x, double *f, double *g);
/* x_out = argmin 1/2 x'Qx + q'x without the box: Quadratic.x_star(), optiml/opti/_base.py:259-269 —
 * cho_solve(cho_factor(Q), -q) on the device (H assembled from the resident panel, blocked MFMA Cholesky); when a pivot
 * is <= 0 (scipy: LinAlgError) the reference's fallback scipy.sparse.linalg.minres(Q, -q)[0] with its defaults (rtol 1e-5,
 * 5 N iterations), one panel product per iteration.  *method: 0 Cholesky, 1 MINRES; *minres_iters: its iteration count.
 * Single-rank contexts, resident panels. */
int bq_problem_x_star(bq_problem *p, double *x_out, int *method, int64_t *minres_iters);
/* out = K w with the raw Gram panel (kernel problems only; n-vectors)  svm/_base.py:877-880 */
int bq_problem_gram_matvec(bq_problem *p, const double *w, double *out);
/* OUT[c] = K W[c], c < k: W and OUT are k x n row-major host arrays, one panel stream per chunk of 4 columns (the k masked
 * products of the one-vs-rest intercepts, svm/_base.py:877-880 once per class).  Single-rank context, resident packed panel.
 * Column c has the same bits whatever the other columns and its position are (not the bits of bq_problem_gram_matvec: agrees to
 * rounding). */
int bq_problem_gram_matmat(bq_problem *p, int k, const double *W, double *out);
/* bq_problem_gram_matmat on the fp64 matrix cores, one panel stream per chunk of 16 columns: the held-out decision values and
 * intercepts of every (fold, C, class) column of a cross-validated search (sklearn GridSearchCV: svm/_base.py:877-880 and
 * decision_function once per fold and candidate).  Column c's bits are a function of W[c] alone (not those of
 * bq_problem_gram_matmat: agrees to rounding). */
int bq_problem_gram_matmat_wide(bq_problem *p, int k, const double *W, double *out);
/* device memory free / in all on the context's device (hipMemGetInfo), and the bytes of the slab that a boxes solver or a wide
 * product allocates for p: what the search's column cap per solve is computed from (GridSearchCV keeps one fit per process) */
int bq_ctx_mem_info(bq_ctx *ctx, int64_t *free_bytes, int64_t *total_bytes);
int64_t bq_problem_wide_slab_bytes(const bq_problem *p);
/* ---- one-vs-one pairs on a class-sorted panel (sklearn OneVsOneClassifier._fit_ovo_binary: SVC.fit once per class pair; the
 * reference's SVC refuses more than two labels, svm/_base.py:231) ---------------------------------------------------------------
 * The panel's rows are sorted by class and every class owns whole 256-row tile rows: class c is tile rows [cls_tiles[c],
 * cls_tiles[c + 1]), cls_tiles[0] = 0, strictly increasing, cls_tiles[ncls] = the panel's tile rows (ceil(n / 256)).  pairs: m
 * pairs (a, b), 2m ints, 0 <= a < b < ncls.  Anything else is BQ_ERR_BADARG.
 * bq_problem_gram_matmat_pairs: OUT[p] = K W[p] on the rows of classes a and b of pair p and exactly 0 on every other row; W[p]
 * outside the pair's rows is never read (the pairs' intercepts, svm/_base.py:877-880 once per pair).  W, OUT: m x n row-major host
 * arrays.  One panel stream for all pairs: an off-diagonal class block is read for its one pair, a class's diagonal block once per
 * 16 pairs containing the class (bq_symmp.hip).  Column p's bits are a function of W[p] and its pair's classes alone (not those of
 * bq_problem_gram_matmat_wide: agrees to rounding).  Single-rank context, resident packed panel. */
int bq_problem_gram_matmat_pairs(bq_problem *p, int ncls, const int *cls_tiles, int m, const int *pairs, const double *W,
                                 double *out);
/* device bytes of the slab of a pair solver / product with these pairs (what the number of pairs per solve is sized from) */
int bq_pairs_slab_bytes(int64_t nb, int ncls, const int *cls_tiles, int m, const int *pairs, int64_t *bytes);
/* the routed product's strips (host only, for inspection): 5 ints per strip (kind: 0 one pair's off-diagonal block, 1 a class's
 * diagonal block; tile row I; first tile J0; tiles; the pair (kind 0) or the class (kind 1)); *count: the number of strips,
 * items == NULL: only *count. */
int bq_pairs_work_list(int64_t nb, int ncls, const int *cls_tiles, int m, const int *pairs, int *items, int64_t cap,
                       int64_t *count);
/* copy rows [row0,row0+nrows) of this rank's resident panel (n columns each) to the host as fp64 */
int bq_problem_panel_rows(bq_problem *p, int64_t row0, int64_t nrows, double *out);
/* time `reps` launches of the panel product with HIP events; returns the mean in ms */
int bq_problem_time_matvec(bq_problem *p, int reps, double *mean_ms);
/* BQ_PLACE_PANEL: how many placements of the panel were timed (0: the flag was not given or did not apply) and the product's
 * launch time on each, in the order tried (ms[0 .. min(*tried, cap))); the panel kept is the fastest of them */
int bq_problem_placement(const bq_problem *p, int *tried, double *ms, int cap);
/* Budget of the BQ_PLACE_PANEL choice for the problems created on this context from now on.  A slow placement costs ~5 % of every
 * product of the solve that follows, so the choice may spend up to 2 % of the products the caller EXPECTS to run
 * (expected_products x the product's measured time), never less than min_ms (< 0: BQ_PLACE_BUDGET_MS, default 200) and never
 * more than max_ms.  SVC / SVR.fit pass their max_iter (svm/_base.py:187-240: the optimizer's iteration cap), a steady-state
 * measurement passes a large number; expected_products = 0 (the default) keeps the fixed min_ms budget.  Candidates that were
 * not kept stay allocated until the first solver created on the problem is destroyed (or the problem, or a device allocation of
 * the library fails): releasing them before the solve slowed it down (profiles/r05/placement_release_transient.txt). */
int bq_ctx_set_placement_budget(bq_ctx *ctx, double min_ms, double max_ms, double expected_products);
/* give the allocations the placement choice is holding back (all of them on this context: up to two panel-sized blocks per problem
 * whose choice tried candidates) to the driver NOW — for a caller that needs the memory for something this library does not see
 * (another allocator in the process, a communicator about to be created).  *bytes (optional): what was released.  The ~0.5 s
 * transient that follows a large release (everything streams 1.5 - 4.5 % slower) is then the caller's. */
int bq_ctx_release_held_memory(bq_ctx *ctx, int64_t *bytes);
/* The Hessian image of a rank-one RBF dual: fl(K + 1) of this rank's tile rows in 6.5 bytes per element, a second allocation beside
 * the compact panel that the one-column product of ProjectedGradient / FrankWolfe streams in the panel's place (every output bit as
 * from the panel).  Built when the first such solver is created on the problem, if the problem is a packed, compact, resident RBF
 * panel with the rank-one term, a tenth of the device stays free beside it and the products announced through
 * bq_ctx_set_placement_budget's expected_products (unknown = 0) repay its allocation and conversion, and if the product, timed on it, is faster than on the panel.  *state: BQ_HIMG_* — built, or
 * why not; *bytes: its size (0 if not built); *build_ms: the conversion; *tried, ms[0 .. min(*tried, cap)): the product's launch time
 * on each allocation tried for it (the placement choice of BQ_PLACE_PANEL, run for the image). */
enum {
    BQ_HIMG_NONE = 0,        /* no ProjectedGradient / FrankWolfe solver was created yet */
    BQ_HIMG_BUILT = 1,
    BQ_HIMG_NOT_ELIGIBLE = 2, /* not (rank-one term, compact, packed, resident), or this rank owns no tile row */
    BQ_HIMG_SWITCHED_OFF = 3, /* test hook hessian_image=0 */
    BQ_HIMG_NO_ROOM = 4,      /* a tenth of the device would not stay free beside it */
    BQ_HIMG_NO_REPAY = 5,     /* expected_products unknown or too few to repay allocation + conversion */
    BQ_HIMG_ALLOC_FAILED = 6,
    BQ_HIMG_OUT_OF_DOMAIN = 7, /* an element of K + 1 could not be encoded: the image was dropped */
    BQ_HIMG_GIVEN_BACK = 8,   /* released when a later device allocation of the library failed */
    BQ_HIMG_NOT_FASTER = 9    /* timed on this problem, the product on the (empty) image was no faster than on the panel: short grids */
};
/* TEST ENTRY (fails with BQ_ERR_BADARG unless BQ_TEST_HOOKS holds product_rows=1): the output vector of the last panel product as the
 * device holds it — *len = nb * 256 entries for a packed panel (the pad rows past n included), n otherwise; out == NULL: only *len */
int bq_problem_last_product(bq_problem *p, double *out, int64_t cap, int64_t *len);
int bq_problem_hessian_image(const bq_problem *p, int *state, int64_t *bytes, double *build_ms, int *tried, double *ms, int cap);

/* ---- solvers (optiml/opti/constrained/, the four .py files) --------------------------------------------------- */
/* lb/ub/x0: dual-dim fp64 host vectors (lb, x0 may be NULL: 0 and mid-box, constrained/_base.py:61-65).
 * eps: stopping accuracy; max_iter: as the reference; fw_t: FrankWolfe trust radius in [0,1).
 * BQ_AS (active_set.py:82-237): same masks, candidate / ratio step, Bland release and tolerances as the reference; the
 * restricted system of line :141 is solved from a Cholesky factor that is KEPT across iterations (the free set moves by
 * one index at a time: the changes are carried through a Schur complement on a base factor, which is rebuilt every 96 to 512
 * changes; hook as_schur=0 re-factorises in every iteration like the reference).  A non-positive pivot takes
 * the reference's minres branch (:142-151). */
int bq_solver_create(bq_problem *p, int kind, const double *lb, const double *ub, const double *x0,
                     double eps, int64_t max_iter, double fw_t, bq_solver **out);
int bq_solver_destroy(bq_solver *s);
/* advance by at most max_steps iterations, device-resident; stats receives one row per evaluated
 * iteration (capacity stats_cap rows, at least max_steps+1).  *status is BQ_STATUS_UNKNOWN while the
 * solver can continue. */
int bq_solver_run(bq_solver *s, int64_t max_steps, bq_iter_stat *stats, int64_t stats_cap,
                  int64_t *n_stats, int *status);
int bq_solver_state(const bq_solver *s, int64_t *iter, int *status, double *f_x);
/* BQ_AS_CG only: relative residual level (default 1e-13) and iteration cap (0 = 2 |A| + 50) of the inner conjugate
 * gradients; total inner iterations so far (0 for the other solvers). */
int bq_solver_set_inner(bq_solver *s, double rtol, int64_t max_iter);
int bq_solver_inner_iters(bq_solver *s, int64_t *total);
/* ActiveSet bookkeeping, totals since the solver was created (0 for the other solvers):
 *   BQ_COUNT_MINRES    iterations whose restricted system Q[A,A] was NOT factorised (non-positive pivot) and took the reference's
 *                      minres branch (active_set.py:142-151) — what a test of the pivot threshold (BQ_AS_PIVOT_REL) looks at
 *   BQ_COUNT_REFACTOR  base-set factorisations of the kept-factor path;  BQ_COUNT_REUSED  iterations solved through a kept factor
 *   BQ_COUNT_INNER     = bq_solver_inner_iters
 *   BQ_COUNT_NO_PRODUCT  ratio-step iterations (active_set.py:152-176) whose f(x) came from the line-search identity
 *                      f(x + t d) = f(x) + (t - t^2/2) g_A'd_A instead of a product with Q (hook as_f_chain=0: none) */
#define BQ_COUNT_INNER 0
#define BQ_COUNT_MINRES 1
#define BQ_COUNT_REFACTOR 2
#define BQ_COUNT_REUSED 3
#define BQ_COUNT_NO_PRODUCT 4
int bq_solver_counter(bq_solver *s, int which, int64_t *value);
int bq_solver_get(bq_solver *s, int what, double *out);

/* ---- batched one-vs-rest ProjectedGradient / FrankWolfe (sklearn OneVsRestClassifier over SVC.fit, svm/_base.py:547-559 once
 * per class, on ONE Gram panel) -----------------------------------------------------------------------------------------------
 * p: a kernel-built BQ_SVC problem (its own labels are not used) on a single-rank context with a resident packed panel (not
 * BQ_STREAM, not BQ_FULL_PANEL): anything else is BQ_ERR_BADARG.  Y: k x n labels (+-1) of the k binary problems; ub: n (shared,
 * lb = 0); x0: k x n or NULL (mid-box); eps, max_iter, fw_t: as bq_solver_create, for every class.  Class c runs the iteration of
 * bq_solver_create(kind) on Q_c = diag(y_c) P diag(y_c) — same formulas, thresholds, stop tests and records; the k products of an
 * iteration are one multi-column panel stream per 4 live classes, and a class that stops leaves the batch.  Class c's iterates
 * have the same bits alone or in any batch.
 * run: at most max_steps iterations of every class still running; stats: k x stats_cap rows (class c at c * stats_cap), n_stats
 * and status: k entries.  get / state: bq_solver_get / bq_solver_state of class cls. */
int bq_msolver_create(bq_problem *p, int kind, int k, const double *Y, const double *ub, const double *x0, double eps,
                      int64_t max_iter, double fw_t, bq_msolver **out);
int bq_msolver_run(bq_msolver *s, int64_t max_steps, bq_iter_stat *stats, int64_t stats_cap, int64_t *n_stats, int *status);
int bq_msolver_state(const bq_msolver *s, int cls, int64_t *iter, int *status, double *f_x);
int bq_msolver_get(bq_msolver *s, int cls, int what, double *out);
int bq_msolver_destroy(bq_msolver *s);
/* The same batched solver with ONE BOX PER COLUMN, for cross-validated searches: sklearn GridSearchCV's per-fold SVC.fit
 * (svm/_base.py:547-559 once per fold, C and class) on ONE Gram panel of all n rows.  UB: k x n (lb = 0): column c = (fold, C,
 * class) has ub = C on the fold's training rows and 0 on its held-out rows, which is the training fold's dual exactly (the held-out
 * entries start at 0 and never move).  Every pass, however few columns are live, takes the 16-column product of
 * bq_problem_gram_matmat_wide, so column c's iterates have the same bits alone, at any position and in any batch.  Y, x0, eps,
 * max_iter, fw_t, run / state / get / destroy: as bq_msolver_create. */
int bq_msolver_create_boxes(bq_problem *p, int kind, int k, const double *Y, const double *UB, const double *x0, double eps,
                            int64_t max_iter, double fw_t, bq_msolver **out);
/* The boxes solver with one column per one-vs-one pair on a class-sorted panel (sklearn OneVsOneClassifier._fit_ovo_binary:
 * SVC.fit on the rows of classes a and b, once per pair; the reference's SVC refuses more than two labels, svm/_base.py:231).
 * cls_tiles, pairs: as bq_problem_gram_matmat_pairs.  Y: m x n labels (+-1); UB: m x n, >= 0 on the rows of the pair's classes and
 * exactly 0 on every other row (else BQ_ERR_BADARG).  Every pass takes the pair-routed product, which streams the panel once for
 * all live pairs; a pair that stops leaves the stream at the next iteration.  Pair p's iterates have the same bits alone, at any
 * position and in any batch.  x0, eps, max_iter, fw_t, run / state / get / destroy: as bq_msolver_create (cls = the pair). */
int bq_msolver_create_pairs(bq_problem *p, int kind, int ncls, const int *cls_tiles, int m, const int *pairs, const double *Y,
                            const double *UB, const double *x0, double eps, int64_t max_iter, double fw_t, bq_msolver **out);
/* The batched solver on k epsilon-insensitive SVR duals (sklearn MultiOutputRegressor over SVR.fit, svm/_base.py:1091-1104 once per
 * target, on ONE Gram panel).  p: a kernel-built BQ_SVR problem on a single-rank context with a resident packed panel (anything else
 * is BQ_ERR_BADARG); its own q is not used.  QL: k x 2n, the linear term of column c ([-y_c; y_c] + epsilon); ub: 2n (shared,
 * lb = 0); x0: k x 2n or NULL (mid-box).  Column c runs the iteration of bq_solver_create(kind) on the SVR problem with linear term
 * QL[c] — same formulas, thresholds, stop tests and records; an iteration's products are one panel stream per 4 live targets of
 * the n-vectors d+ - d-, and a target that stops leaves the batch.  Target c's iterates have the same bits alone, at any position
 * and in any batch (they agree with bq_solver_create's to rounding: another product kernel).  eps, max_iter, fw_t, run / state /
 * get / destroy: as bq_msolver_create, on vectors of 2n (cls = the target). */
int bq_msolver_create_svr(bq_problem *p, int kind, int k, const double *QL, const double *ub, const double *x0, double eps,
                          int64_t max_iter, double fw_t, bq_msolver **out);
/* The SVR batch with ONE BOX PER COLUMN, for cross-validated searches over C and epsilon: sklearn GridSearchCV's per-fold SVR.fit
 * on ONE Gram panel of all n rows.  QL: k x 2n, column c = (fold, C, epsilon) has [-y; y] + epsilon; UB: k x 2n, >= 0: C on both
 * halves of the fold's training rows and 0 on both halves of its held-out rows, which is the training fold's dual exactly (those
 * entries start at 0 and never move).  Row i is held out for column c exactly when UB[c][i] == 0 and UB[c][n + i] == 0; a row with
 * exactly one half zero is BQ_ERR_BADARG.  Every pass takes the 16-column product, so column c's iterates have the same bits alone,
 * at any position and in any batch.  p, x0, eps, max_iter, fw_t, run / state / get / destroy: as bq_msolver_create_svr. */
int bq_msolver_create_svr_boxes(bq_problem *p, int kind, int k, const double *QL, const double *UB, const double *x0,
                                double eps, int64_t max_iter, double fw_t, bq_msolver **out);
/* Held-out scores of every column of a bq_msolver_create_svr_boxes solver (any other solver: BQ_ERR_BADARG), from its state on the
 * device, after any run: no k x n array crosses the bus.  y: n targets; epsilon: k.  Per column, with coef = x+ - x- on the support
 * rows (x+ or x- above 1e-6, SVR.fit's threshold) and u = K coef (one 16-column product per 16 columns):
 *   n_sv       the support rows;        intercept  (sum over them of (y - u) - epsilon) / n_sv, SVR.fit's order of operations
 *   n_held     the held-out rows;       sse        sum over them of (y - (u + intercept))^2
 * Every sum has a fixed order and reads its own column only, so a column's results have the same bits in any batch.  n_sv = 0 gives
 * intercept = sse = NaN (SVR.fit divides by zero there). */
int bq_msolver_svr_heldout(bq_msolver *s, const double *y, const double *epsilon, double *intercept, int64_t *n_sv, double *sse,
                           int64_t *n_held);

/* ---- nu-one-class duals on a capped simplex (sklearn.svm.OneClassSVM, Schoelkopf et al.; libsvm's ONE_CLASS) ------------------
 * Column c solves  min 1/2 x'Kx  s.t.  0 <= x <= UB[c], sum x = mass[c]  on the Gram panel of p, a kernel-built BQ_PLAIN problem
 * without a diagonal term on a single-rank context with a resident packed panel (anything else is BQ_ERR_BADARG).  OneClassSVM is
 * UB = 1, mass = nu n (libsvm's scaling: the solution is sklearn's dual_coef_); a row with UB[c][i] = 0 is a row the column does
 * not train on.  The equality row is kept (without it x = 0 is optimal), so the step is the Euclidean projection onto the capped
 * simplex, P(v) = clip(v - tau, 0, u) with sum P = mass, inside a nonmonotone spectral projected-gradient loop:
 *   x = P(0) (or x0); g = K x; f = 1/2 x'g; s = 1; at the top of iteration it
 *     viol = max_{x_i > 0} g_i - min_{x_i < u_i} g_i over the rows with u_i > 0 (libsvm's maximal violating pair; -inf if a set is empty)
 *     record (it, f, r1 = viol, r2 = the last step length a, r3 = s); viol <= tol: optimal; it == max_iter: stopped
 *     d = P(x - s g) - x; g'd >= 0: optimal; a = 1 if f + g'd + 1/2 d'Kd <= max(the last 10 f) + 1e-4 g'd, else -g'd / d'Kd
 *     x += a d; g += a K d; f += a g'd + 1/2 a^2 d'Kd; s = clamp(d'd / d'Kd, 1e-10, 1e10), 1e10 where d'Kd <= 0
 * so tol is sklearn.svm.OneClassSVM's tol.  An iteration's products are one panel stream per 16 live columns (the product of
 * bq_problem_gram_matmat_wide); a column that stops leaves the stream.  Column c's iterates and records have the same bits alone,
 * at any position and in any batch.
 * UB: k x n, in [0, 2^1021]; mass: k, 0 < mass[c] <= sum UB[c] (a mass within n roundings of the sum is the whole box, the single
 * point x = UB[c]); x0: k x n inside its set, or NULL (P(0)); tol >= 0; max_iter > 0.  A NULL argument, k < 1 or any of the above
 * violated: BQ_ERR_BADARG.  run / state / get / destroy: as bq_msolver_create (a run of max_steps iterations writes at most
 * max_steps records per column).
 * bq_msolver_simplex_offsets: libsvm's calculate_rho of every column from its state on the device, after a run, over the rows with
 * UB > 0 and with exact comparisons: rho = the mean of g over the free rows (0 < x < UB), summed in index order; without a free
 * row (min_{x = 0} g + max_{x = UB} g) / 2.  n_sv: the rows with x > 0; n_free: the free rows.  k entries each.
 * bq_simplex_project: P[c] = the projection of V[c] onto {0 <= p <= UB[c], sum p = mass[c]}, k x n host arrays, by the solver's
 * projection kernel: one workgroup per column, tau by an 8-section search on the sum that ends exactly on the linear piece holding
 * the root (|V| at most 2^1021, so that the first bracket's width is finite; else BQ_ERR_BADARG).  0 <= P <= UB holds bitwise, P = 0 where UB = 0, and row c's bits depend on (V[c], UB[c], mass[c]) alone. */
int bq_msolver_create_simplex(bq_problem *p, int k, const double *UB, const double *mass, const double *x0, double tol,
                              int64_t max_iter, bq_msolver **out);
int bq_msolver_simplex_offsets(bq_msolver *s, double *rho, int64_t *n_sv, int64_t *n_free);
int bq_simplex_project(bq_ctx *ctx, int k, int64_t n, const double *V, const double *UB, const double *mass, double *P);

/* ---- nu-SVC and nu-SVR duals on two capped simplices (sklearn.svm.NuSVC / NuSVR; libsvm's solve_nu_svc / solve_nu_svr) ------------
 * Column c solves  min 1/2 b'Kb + q'x  over m variables in two disjoint groups, group t being the capped simplex
 * {0 <= x <= UB on its variables, sum x = mass[c][t]}, with b = sum_j s_j x_j scattered to panel row j mod n and gradient
 * g_j = q_j + s_j (K b)_{j mod n}.  The two equality rows of the nu-duals (sum s x = 0, sum x = R) are these two masses, R / 2 each,
 * and the projection onto the product of the two sets is the two one-group projections taken independently.
 *   BQ_SX_LABELS  m = n, s = S[c] (+-1 per row), group 0 the rows with S = +1, group 1 those with S = -1.  nu-SVC: UB = 1 on the
 *                 training rows, mass = nu n / 2 twice, q NULL.  A row with UB = 0 is not trained on and its S is not read.
 *   BQ_SX_PAIRED  m = 2n, s = +1 on j < n (group 0) and -1 on j >= n (group 1); S is NULL.  nu-SVR: UB = C, mass = C nu n / 2 twice,
 *                 q = (-y, +y).
 * The iteration is bq_msolver_create_simplex's with f = 1/2 x'(g - q) + q'x at the start, d'Kd = sum_j d_j s_j (K e)_{j mod n} for
 * the folded direction e (LABELS: S o d; PAIRED: d_i - d_{n + i}), one n-row product per iteration for either layout, and the
 * violation libsvm's Solver_NU measure: the maximum over the two groups of the group's maximal-violating-pair value (-inf for a
 * group with an empty side).  The problem is as for bq_msolver_create_simplex.  UB: k x m in [0, 2^1021]; mass: k x 2 with
 * 0 < mass[c][t] <= the sum of group t's box (within n roundings of it: the whole box); a group without a row of positive box,
 * an S entry other than +-1 on a row with UB > 0, a non-finite q or an x0 (k x m) outside its set: BQ_ERR_BADARG.  Column c's
 * iterates and records have the same bits alone, at any position and in any batch; bq_msolver_get hands out m entries.
 * bq_msolver_simplex2_offsets: libsvm's Solver_NU::calculate_rho after a run: r_t = the mean of g over group t's free rows, summed
 * in index order, else (min_{x = 0} g + max_{x = UB} g) / 2 over the group; r1, r2: k each; n_sv, n_free: k x 2 (the group's rows
 * with x > 0 and its free rows).  The caller forms r = (r1 + r2) / 2 and rho = (r1 - r2) / 2. */
enum { BQ_SX_LABELS = 0, BQ_SX_PAIRED = 1 };
int bq_msolver_create_simplex2(bq_problem *p, int k, int layout, const double *S, const double *UB, const double *mass,
                               const double *q, const double *x0, double tol, int64_t max_iter, bq_msolver **out);
int bq_msolver_simplex2_offsets(bq_msolver *s, double *r1, double *r2, int64_t *n_sv, int64_t *n_free);
/* Held-out scores of every column of a bq_msolver_create_simplex2 solver that has run (a NULL argument, any other solver — the
 * one-group and the pair-routed simplex solvers included — or a solver before its first run: BQ_ERR_BADARG), from its state on the
 * device: sklearn GridSearchCV's per-fold NuSVC / NuSVR score of a column whose box is 0 on the fold's held-out rows, and no k x n
 * array crosses the bus.  y: n entries; BQ_SX_LABELS: the labels of all rows, each exactly +-1 (the solver's own S is not read on
 * held-out rows, so they come in here); BQ_SX_PAIRED: the targets, all finite; anything else is BQ_ERR_BADARG.
 *   r1, r2 (k), n_sv, n_free (k x 2)   the bits of bq_msolver_simplex2_offsets on the same state
 *   u = K b, b the signed, folded x (S o x; x_i - x_{n + i}), by one 16-column product per 16 columns, every column in its own slot,
 *   live or not; the solver's incrementally updated g is not read.  rho = (r1 - r2) / 2, r = (r1 + r2) / 2
 *   n_held (k)      the held-out rows: UB[c][i] == 0 (LABELS), both halves 0 (PAIRED)
 *   n_correct (k)   LABELS: the held-out rows whose prediction, +1 exactly when (u_i - rho) / r > 0 in that form (NuSVC.predict: a
 *                   NaN or a non-positive r predicts as np.where(decision > 0, ...) does), equals y_i; PAIRED: 0
 *   sse (k)         PAIRED: the sum over the held-out rows of (y_i - (u_i - rho))^2 (NuSVR.predict is u - rho); LABELS: 0
 * One workgroup per column sums in a fixed order and reads its own column only, so a column's results have the same bits alone, at
 * any position and in any batch.  The solver's state and liveness are untouched: a later run continues as without the call. */
int bq_msolver_simplex2_heldout(bq_msolver *s, const double *y, double *r1, double *r2, int64_t *n_sv, int64_t *n_free,
                                int64_t *n_held, int64_t *n_correct, double *sse);
/* The two-group columns of one-vs-one nu-SVC on a class-sorted panel (sklearn OneVsOneClassifier(NuSVC): NuSVC.fit on the rows of
 * classes a and b, once per pair and nu), with the pair-routed product of bq_msolver_create_pairs.  cls_tiles, pairs: as
 * bq_problem_gram_matmat_pairs; the same pair may appear in several columns (one per nu).  Column c of pair (a, b), a < b, has m = n
 * variables in panel order; group 0 is the row range of class b with s = +1 (OneVsOneClassifier makes the larger label positive),
 * group 1 the row range of class a with s = -1; there is no S and no linear term.  UB: m x n, >= 0 on the rows of the pair's classes
 * and exactly 0 on every other row (a class's ghost rows and held-out rows have UB = 0 too); mass: m x 2, one per group, as
 * bq_msolver_create_simplex2; x0: m x n inside its set, or NULL.  nu-SVC of pair (a, b): UB = 1 on the pair's data rows,
 * mass = nu (n_a + n_b) / 2 twice.  The iteration, the stop test and the records are bq_msolver_create_simplex2's; every pass takes
 * the routed product, which streams the panel at most once for all live columns and reads and writes a column on its pair's rows
 * only, and a column's own kernels walk the rows of its two classes only: x, d and g stay exactly 0 on every other row.  Column c's
 * iterates and records have the same bits alone, at any position and in any batch.  A NULL argument or m < 1 (checked first), a
 * problem other than bq_msolver_create_simplex's, bad cls_tiles or pairs, a group without a row of positive box, a mass above its
 * group's box or an x0 outside its set: BQ_ERR_BADARG.  run / state / get / destroy: as bq_msolver_create (cls = the column; get
 * hands out n entries); bq_msolver_simplex2_offsets takes the solver as it takes bq_msolver_create_simplex2's. */
int bq_msolver_create_simplex2_pairs(bq_problem *p, int ncls, const int *cls_tiles, int m, const int *pairs, const double *UB,
                                     const double *mass, const double *x0, double tol, int64_t max_iter, bq_msolver **out);

/* ---- Platt calibration (sklearn CalibratedClassifierCV(method='sigmoid'): calibration.py _sigmoid_calibration, once per (fold,
 * class)) -----------------------------------------------------------------------------------------------------------------------
 * bq_platt_fit: ncal sigmoid fits p = 1 / (1 + exp(A f + B)) in one launch, one workgroup each.  D, L: ncal x n host arrays;
 * D[j] the decision values of calibrator j, L[j] its labels: > 0 positive, < 0 negative, 0 a row that is not in its sample and enters
 * no sum.  The iteration is libsvm's sigmoid_train (Lin, Lin & Weng 2007): targets (N+ + 1) / (N+ + 2) and 1 / (N- + 2), start
 * A = 0, B = log((N- + 1) / (N+ + 1)), Newton's direction with 1e-12 on the Hessian's diagonal, step halving while
 * f_new >= f + 1e-4 step g'd down to a step of 1e-10, stop when both gradient entries are below 1e-5, at most 100 iterations.
 * Per calibrator: A, B, iters (Newton steps taken), loss (the final value), n_pos, n_neg, flags (BQ_PLATT_*: libsvm's two
 * warnings; the values at that point are returned).  A calibrator without a labelled row gets A = B = 0 and BQ_PLATT_EMPTY.
 * Every sum has a fixed order and reads its own calibrator only: (A, B) have the same bits alone, at any position, in any batch.
 * ncal < 1, n < 1 or a NULL pointer: BQ_ERR_BADARG. */
#define BQ_PLATT_LINE_SEARCH 1 /* the line search failed (the step fell below 1e-10) */
#define BQ_PLATT_MAX_ITER 2    /* the iteration cap was reached */
#define BQ_PLATT_EMPTY 4       /* no labelled row */
int bq_platt_fit(bq_ctx *ctx, int ncal, int64_t n, const double *D, const double *L, double *A, double *B, int *iters, double *loss,
                 int64_t *n_pos, int64_t *n_neg, int *flags);
/* Held-out decision values and Platt fits of the columns of a bq_msolver_create_boxes solver (any other solver: BQ_ERR_BADARG),
 * from its state on the device, after any run.  cal_of: k ints, column c's calibrator in [0, ncal) or -1 for a column that feeds
 * none (a fit on all the data).  Per column, with coef = x y on the support rows (x above 1e-6, SVC.fit's threshold) and u = K coef
 * (one 16-column product per 16 columns):
 *   n_sv       the support rows;        intercept  (sum over them of (y - u)) / n_sv, SVC.fit's order of operations (n_sv = 0: NaN)
 * and on the column's held-out rows (UB[c][i] == 0) the decision value u + intercept and the label y go to row cal_of[c] of two
 * zeroed ncal x n device buffers, on which bq_platt_fit's kernel runs: A, B, iters, loss, n_pos, n_neg, flags have ncal entries.
 * Columns that share a calibrator must have disjoint held-out rows (else BQ_ERR_BADARG).  dec: NULL, or ncal x n, which receives
 * the decision buffer (0 on the rows no column of the calibrator holds out). */
int bq_msolver_svc_heldout(bq_msolver *s, int ncal, const int *cal_of, double *intercept, int64_t *n_sv, double *A, double *B,
                           int *iters, double *loss, int64_t *n_pos, int64_t *n_neg, int *flags, double *dec);
/* bq_msolver_svc_heldout for the columns of a bq_msolver_create_pairs solver (any other solver: BQ_ERR_BADARG): the folds of a
 * one-vs-one calibration, column (pair, fold) with UB = 0 on the fold's held-out rows of the pair's classes.  data_row: n bytes, 1 a
 * data row, 0 a ghost row of the class-sorted panel.  Per column coef, n_sv and intercept as there, with u = K coef by ONE pair-routed
 * product over all columns, every pair live as in bq_problem_gram_matmat_pairs (the solver's own liveness is restored from its
 * columns' states: a later run continues as if this call had not been made).  Column c's held-out rows are the data rows of its pair's
 * two classes with UB[c][i] == 0 — never a ghost row, never a row of another class; each writes u + intercept and its label to row
 * cal_of[c] of the two zeroed ncal x n buffers.  cal_of, the disjointness rule (on those rows), n_sv = 0, the Platt outputs and dec:
 * as bq_msolver_svc_heldout.  Every sum has a fixed order and reads its own column only: a column's results have the same bits in
 * any batch. */
int bq_msolver_pairs_heldout(bq_msolver *s, const unsigned char *data_row, int ncal, const int *cal_of, double *intercept,
                             int64_t *n_sv, double *A, double *B, int *iters, double *loss, int64_t *n_pos, int64_t *n_neg,
                             int *flags, double *dec);

/* ---- one-vs-one vote (sklearn OneVsOneClassifier.predict: multiclass.py _ovr_decision_function and argmax, once per test row; a
 * GridSearchCV over a one-vs-one SVC evaluates it on every fold's held-out rows) --------------------------------------------------
 * bq_ovo_vote: t rows of P = ncls (ncls - 1) / 2 pair decision values, D t x P row-major (host), the pairs in the order (0,1),
 * (0,2), ..., (1,2), ..., positive towards the pair's larger class.  Per row, for k = 0..P-1 over the pairs (i, j) in that order:
 * conf[i] -= D[k]; conf[j] += D[k]; votes[D[k] > 0 ? j : i] += 1; then Y[c] = votes[c] + conf[c] / (3 (|conf[c]| + 1)), evaluated
 * without fused multiply-adds and with IEEE division, so Y has the bits of the NumPy statements.  pred[row] is np.argmax of the row's
 * Y: the first NaN if there is one, else the first maximum.  With ncls = 2 that is OneVsOneSVC.predict's class, 1 exactly when
 * Y[1] > 0.  pred: t ints; Y: NULL, or t x ncls, which receives the decision matrix.  One thread per row, no atomics: a row's
 * result depends on that row alone.  ncls < 2, ncls > 64, t < 1 or a NULL ctx / D / pred: BQ_ERR_BADARG, before any device call. */
int bq_ovo_vote(bq_ctx *ctx, int ncls, int64_t t, const double *D, int *pred, double *Y);
/* Held-out accuracy of the (candidate, fold) groups of a bq_msolver_create_pairs solver (any other solver: BQ_ERR_BADARG), from its
 * state on the device, after any run: sklearn GridSearchCV's per-fold score of a one-vs-one SVC, and no columns x n array crosses
 * the bus.  group_of: k ints in [0, ngroups); every group holds every pair of the ncls classes exactly once, so k = ngroups x P
 * (else BQ_ERR_BADARG).  data_row: n bytes, 1 a data row, 0 a ghost row.  held: ngroups x n bytes, 1 a row the group scores; such a
 * row must be a data row and must have UB = 0 in every column of its group — it was not trained on — else BQ_ERR_BADARG (checked
 * on the host against the solver's copy of the boxes; a box is 0 on ghost rows and on the rows of other classes too, so the held-out
 * rows cannot be read off the boxes).
 * Per column: coef, n_sv and intercept exactly as bq_msolver_svc_heldout forms them (n_sv = 0: NaN), with u = K coef by the
 * 16-column product, every column in its own slot, live or not, in scratch of the call's own — u on ALL rows, where the routed
 * product leaves 0 outside the pair's classes.
 * Per group: n_held, the held rows; every held row votes as bq_ovo_vote's rows do on conf_k = u_k[row] + intercept_k over the
 * group's P columns in pair order; n_correct, the held rows whose predicted class is the class whose tile rows (cls_tiles) hold the
 * row; a group with a NaN intercept reports n_correct = -1 (a failed fit).  pred: NULL, or ngroups x n ints, the predicted class on
 * the held rows and -1 elsewhere.  Integer sums in a fixed order: a group's results have the same bits alone, at any position and in
 * any batch.  The solver's state, buffers and liveness are untouched: a later run continues as without the call. */
int bq_msolver_pairs_vote_heldout(bq_msolver *s, const unsigned char *data_row, int ngroups, const int *group_of,
                                  const unsigned char *held, double *intercept, int64_t *n_sv, int64_t *n_held,
                                  int64_t *n_correct, int *pred);

/* ---- checkpoint / resume (SURVEY 5 "checkpoint / resume") -------------------------------------------------------
 * What the reference's loop holds at the TOP of an iteration, so that a run which was stopped (max_iter, a callback's
 * StopIteration, a process that has to go) can be continued in a NEW solver: the reference offers `x=` only
 * (constrained/_base.py:61-65) and keeps the rest as locals — InteriorPoint's multipliers lp / lm (interior_point.py:181-186),
 * ActiveSet's masks L / U (active_set.py:91-92), FrankWolfe's best lower bound (frank_wolfe.py:90,105-106), self.g_x.
 *
 * bq_solver_get_state: the state at the top of the NEXT iteration (iteration `iter`): a step that has been decided but not yet
 * applied to the device vectors (PG / FW: x + t d, g + t Qd; IP: x + t dx, lp + t dlp, lm + t dlm) is applied to the copies
 * handed out, with the device's own rounding (one rounded product, one sum; PG / FW: x then kept in [lb, ub], as the device keeps
 * it: the step is feasible and only its rounding can pass a bound).  Vector pointers that are NULL are skipped; `have`
 * says which of the others were filled (BQ_STATE_*): lp / lm exist for BQ_IP, the masks (1.0 / 0.0 per index) for BQ_AS / BQ_AS_CG.
 *
 * bq_solver_set_state: into a solver that has not run yet (same problem, kind, bounds).  x is required; g, lp & lm, the masks are
 * taken when given (`have`), otherwise formed as the reference forms them at a start point (g = Qx + q by one product, lp / lm
 * from g, empty masks).  With everything given, InteriorPoint, ProjectedGradient and FrankWolfe continue BIT-IDENTICALLY to the
 * run that was stopped (every later quantity is a function of this state); ActiveSet continues from the same point and masks with a
 * freshly built factor (the stopped run's was updated incrementally: same iterates to rounding).
 * max_iter keeps counting from `iter`. */
#define BQ_STATE_X 1
#define BQ_STATE_G 2
#define BQ_STATE_MULT 4   /* lp and lm */
#define BQ_STATE_MASKS 8  /* mask_l and mask_u */
typedef struct bq_solver_snapshot {
    int64_t iter;      /* iterations completed = index of the next iteration record */
    int kind;          /* BQ_PG ... (get: filled; set: must match the solver, or -1 = not checked) */
    int have;          /* BQ_STATE_* bits: which vectors are filled (get) / given (set) */
    double f;          /* objective of the last record (NaN before the first); informational on set */
    double best_lb;    /* FrankWolfe: best lower bound so far (-inf before the first record) */
    double *x, *g, *lp, *lm, *mask_l, *mask_u;   /* dual-dim fp64 host vectors owned by the caller, NULL = absent */
} bq_solver_snapshot;
int bq_solver_get_state(bq_solver *s, bq_solver_snapshot *state);
int bq_solver_set_state(bq_solver *s, const bq_solver_snapshot *state);

/* ---- augmented-Lagrangian dual + first-order update rules ------------------------------------
 * min 1/2 x'Qx + q'x  s.t.  a_eq'x = 0 (optional), lb <= x <= ub (each optional), relaxed into
 *   L(x) = f(x) + dual'c(x) + rho/2 |[c_eq; max(c_in, 0)]|^2,  c = [a_eq'x; lb - x; x - ub]
 * (AugmentedLagrangianQuadratic, optiml/opti/constrained/_base.py:224-410) and minimised by one of the reference's
 * full-batch "stochastic" rules (optiml/opti/unconstrained/stochastic/, the seven rule files) with the multiplier update and stop tests
 * of optiml/opti/_base.py:129-146.  This is the SVC/SVR dual branch for unconstrained optimizers
 * (optiml/ml/svm/_base.py:638-723, :1188-1270), including reg_intercept=False (equality row y / [1;-1]).
 * Records: f = L(x), r1 = primal value f(x), r2 = |c(x_new)|_2, r3 = |d dual|_2 + |d x|_2 (the two stop-test values).
 * With no constraint at all (a_eq = lb = ub = NULL) it is the plain rule on the quadratic: runs `epochs` iterations. */
enum { BQ_RULE_SGD = 0, BQ_RULE_ADAM = 1, BQ_RULE_AMSGRAD = 2, BQ_RULE_ADAMAX = 3, BQ_RULE_ADAGRAD = 4,
       BQ_RULE_ADADELTA = 5, BQ_RULE_RMSPROP = 6 };
enum { BQ_MOM_NONE = 0, BQ_MOM_POLYAK = 1, BQ_MOM_NESTEROV = 2 };
typedef struct bq_al_params {
    int32_t rule, momentum_type;   /* AdaGrad and AdaDelta have no momentum (the reference classes take none) */
    double step_size, momentum;    /* constants; per-iteration schedules: bq_al_solver_set_schedules */
    double beta1, beta2;           /* Adam, AMSGrad, AdaMax */
    double decay;                  /* AdaDelta, RMSProp */
    double offset;
    double rho, tol;               /* penalty (> 0); tolerance of the two stop tests */
    int64_t epochs;                /* full batch: one epoch per iteration; 'stopped' when reached */
} bq_al_params;
/* x0 is required (the reference draws it uniform(0,1): optiml/opti/_base.py:36-57 — host side); dual0 (layout of
 * BQ_GET_DUAL) may be NULL = zeros.  The returned solver is driven by bq_solver_run / _state / _get / _destroy. */
int bq_al_solver_create(bq_problem *p, const bq_al_params *prm, const double *a_eq, const double *lb,
                        const double *ub, const double *x0, const double *dual0, bq_solver **out);
/* optional schedules (stochastic/schedules.py; the reference draws one value per iteration from an iterable step_size /
 * momentum): entry k is used by iteration k, the last entry continues; either pointer may be NULL.  Before the first run. */
int bq_al_solver_set_schedules(bq_solver *s, const double *step_sizes, const double *momenta, int64_t count);
/* number of multipliers (length of BQ_GET_DUAL) */
int bq_al_solver_dual_size(const bq_solver *s, int64_t *n_dual);
/* The batch of k augmented-Lagrangian solvers on ONE Gram panel: sklearn OneVsRestClassifier over SVC.fit and
 * MultiOutputRegressor over SVR.fit on the stochastic-optimizer branch (optiml/ml/svm/_base.py:638-723, :776-860 once per class;
 * :1188-1270, :1330-1415 once per target) — the only box-type route to reg_intercept=False (equality row y_c / [1; -1]) and to the
 * squared losses (diag = 1/(2C), no upper bound).  p: a kernel-built BQ_SVC or BQ_SVR problem on a single-rank context with a
 * resident packed panel (anything else is BQ_ERR_BADARG); its own labels are not used.  Column c is the solver that
 * bq_al_solver_create(p, prm, a_eq_c, lb, ub, x0_c, dual0_c) makes, with Q_c = diag(y_c) P diag(y_c) (BQ_SVC, Y: k x n labels +-1)
 * or the linear term QL[c] (BQ_SVR, QL: k x 2n; NULL: every column has p's q) — same formulas, rules, multiplier update, stop tests
 * and records (optiml/opti/_base.py:129-146 and the seven rule files); an iteration's products are one panel stream per 4 live
 * columns, and a column that stops leaves the batch.  Column c's iterates have the same bits alone, at any position, in any batch
 * and however the iterations are cut into runs (they agree with bq_al_solver_create's to rounding: another product kernel).
 * a_eq: NULL (no equality row), one row of N for every column (a_ld = 0) or one per column (a_ld = N); lb, ub: N each or NULL,
 * shared; x0: k x N (required); dual0: k x n_dual in the layout of BQ_GET_DUAL, or NULL = zeros.  Constant step size and momentum;
 * momentum none or Polyak: BQ_MOM_NESTEROV is BQ_ERR_BADARG (it needs a jump and a close per iteration), and there are no
 * schedules.  run / state / get / destroy: as bq_msolver_create, on vectors of N; get takes BQ_GET_DUAL, _X, _X_NOW, _G, _D per
 * column as bq_solver_get does for an augmented-Lagrangian solver. */
int bq_msolver_create_al(bq_problem *p, const bq_al_params *prm, int k, const double *Y, const double *QL, const double *a_eq,
                         int64_t a_ld, const double *lb, const double *ub, const double *x0, const double *dual0,
                         bq_msolver **out);

/* ---- SMO on the resident Gram panel (optiml/ml/svm/smo.py) -----------------------------------------
 * SMOClassifier (:99-357) / SMORegression (:386-797): the reg_intercept=False duals through SVC/SVR(optimizer='smo')
 * (optiml/ml/svm/_base.py:560-573, :1106-1120).  `p` is a kernel-built problem of n samples (only its Gram panel K is
 * used; single-rank contexts); y: labels in {+1,-1} (BQ_SVC) or targets (BQ_SVR).  One call of bq_smo_run advances
 * by at most max_outer outer iterations (one sweep over the samples each, smo.py:327-351) and reports the total
 * number done and whether the loop has terminated.  Ties between free samples with bit-identical cached errors are
 * resolved towards the smaller index (the reference: CPython set order) — see oracle/smo_oracle.py. */
typedef struct bq_smo bq_smo;
enum { BQ_SMO_ALPHAS = 0,   /* n (BQ_SVC) or [alpha+; alpha-] 2n (BQ_SVR) */
       BQ_SMO_ERRORS = 1,   /* n: the error cache */
       BQ_SMO_SCALARS = 2,  /* 6: b_up, b_low, b_up_idx, b_low_idx, successful pair steps, intercept b */
       BQ_SMO_STATS = 3     /* 4: helper workgroups per full sweep, error sums they delivered, sums rejected because the list
                             * entries read did not hash to the published value, results rejected by their own checksum —
                             * the two rejection counts are self-checks of the inter-workgroup hand-off and must be 0 */ };
int bq_smo_create(bq_problem *p, int task, const double *y, double C, double epsilon, double tol, bq_smo **out);
/* bq_smo_create with a box per row: 0 <= alpha_i <= Cw[i], Cw[i] = C * sample_weight_i * class_weight[y_i] — what libsvm and
 * sklearn.svm.SVC / SVR(class_weight=, fit(sample_weight=)) solve; the reference (smo.py:99-357, :386-797) has the one C only.
 * Index 2 the examined sample, 1 its partner (smo.py:130-224 / :447-600): membership of row i in the free / up / low sets
 * (classification) and its kind and clipping (regression) use Cw[i]; the pair bounds are
 *   BQ_SVC  y1 != y2: L = max(0, a2 - a1), H = min(C2, C1 + a2 - a1);  y1 == y2: L = max(0, a2 + a1 - C1), H = min(C2, a2 + a1);
 *           the new multipliers snap to their own box: n > C - 1e-8 C ? C : (n <= 1e-8 C ? 0 : n), C2 for n2 and C1 for n1;
 *   BQ_SVR  (p1, p2): L = max(0, g - C1), H = min(C2, g);        (p1, m2): L = max(0, -g), H = min(C2, C1 - g);
 *           (m1, p2): L = max(0, g), H = min(C2, C1 + g);        (m1, m2): L = max(0, -g - C1), H = min(C2, -g),
 *           g = (p1 - m1) + (p2 - m2).
 * With C1 == C2 each is bq_smo_create's expression operation for operation: on a constant vector Cw = C the solver has the
 * bits of bq_smo_create(p, task, y, C, epsilon, tol), with or without helper workgroups (they form sums over the support list
 * and never read a box).  Cw: n, every entry finite and > 0, else BQ_ERR_BADARG before any device call; a 7-byte (compact)
 * panel is BQ_ERR_BADARG too.  Everything else — run, get, destroy, the other argument checks — as bq_smo_create. */
int bq_smo_create_weighted(bq_problem *p, int task, const double *y, const double *Cw, double epsilon, double tol, bq_smo **out);
int bq_smo_run(bq_smo *s, int64_t max_outer, int64_t *outer_iters, int *finished);
int bq_smo_get(bq_smo *s, int what, double *out);
int bq_smo_destroy(bq_smo *s);

/* ---- batched SMO: k duals on one Gram panel, one walker workgroup per column ----------------------------------------
 * What OneVsRestClassifier(SVC(optimizer='smo')) / MultiOutputRegressor(SVR(optimizer='smo')) and GridSearchCV over them do by
 * one SMOClassifier / SMORegression per column (optiml/ml/svm/smo.py:99-357, :386-797 through svm/_base.py:560-573, :1106-1120),
 * each on a Gram matrix of its own.  Column c is the solver bq_smo_create(p, task, Y[c], C[c], epsilon[c], tol) makes, run without
 * helper workgroups: same sweeps, same tie rule, same summation order, so its multipliers, error cache, thresholds and counts have
 * the bits of that solver whatever the other columns do, in any batch and however the outer iterations are cut into runs.
 * p: as bq_smo_create (kernel-built, resident panel, single-rank context).  Y: k x n labels +-1 (BQ_SVC) or targets (BQ_SVR);
 * C: k; epsilon: k, or NULL (0); row_ptr / rows: NULL, or per column an ascending list rows[row_ptr[c] .. row_ptr[c + 1]) of the
 * panel rows it trains on (the training rows of a cross-validation fold) — the column is then the solver of the sub-problem on those
 * rows (its first listed +1 / -1 rows, or its first listed target, start the thresholds) and every other row keeps multiplier 0.
 * BQ_ERR_BADARG: a streamed or non-kernel problem, world > 1, a list that is not strictly ascending or leaves [0, n), a list (or n)
 * shorter than 2, a BQ_SVC column without both labels among its rows, C <= 0, epsilon < 0, tol <= 0 — all before any device call.
 * Device memory: about 36 n (BQ_SVC) / 44 n (BQ_SVR) bytes per column. */
typedef struct bq_msmo bq_msmo;
int bq_msmo_create(bq_problem *p, int task, int k, const double *Y, const double *C, const double *epsilon, double tol,
                   const int64_t *row_ptr, const int32_t *rows, bq_msmo **out);
/* bq_msmo_create with a box per column and row: CW is k x n and column c is the solver bq_smo_create_weighted(p, task, Y[c],
 * CW[c], epsilon[c], tol) makes (formulas there), run without helper workgroups — what OneVsRestClassifier /
 * OneVsOneClassifier(SVC(class_weight='balanced')) do by one weighted libsvm fit per column.  A column whose row of CW is
 * constant has the bits of the bq_msmo_create column with that C; a weighted column has the bits of the weighted single solver,
 * at any position, beside any other columns and however the outer iterations are cut into runs.  On a row a column trains on
 * (every row without row lists) CW must be finite and > 0, else BQ_ERR_BADARG before any device call; entries on rows outside
 * a column's list are never read (they may be NaN).  A 7-byte (compact) panel is BQ_ERR_BADARG.  Everything else — the other
 * arguments and their checks, run, get, destroy, bq_msmo_vote_heldout / _svr_heldout / _svc_heldout, which read multipliers,
 * labels and the walkers' records only — as bq_msmo_create.  Device memory: 8 n more bytes per column. */
int bq_msmo_create_weighted(bq_problem *p, int task, int k, const double *Y, const double *CW, const double *epsilon, double tol,
                            const int64_t *row_ptr, const int32_t *rows, bq_msmo **out);
/* At most max_outer launches; each advances every column still running by one outer iteration (smo.py:327-351 / :764-789), finished
 * columns are not launched.  outer / finished / failed: k each — outer iterations done, the loop has terminated, and the walker
 * met the reference's 'unexpected status' (smo.py:270-271, :756: such a column is finished too; the others go on). */
int bq_msmo_run(bq_msmo *s, int64_t max_outer, int64_t *outer, int *finished, int *failed);
/* column c's BQ_SMO_ALPHAS / BQ_SMO_ERRORS / BQ_SMO_SCALARS, as bq_smo_get (there are no helpers: BQ_SMO_STATS is BQ_ERR_BADARG) */
int bq_msmo_get(bq_msmo *s, int c, int what, double *out);
int bq_msmo_destroy(bq_msmo *s);
/* Held-out accuracy of the (candidate, fold) groups of a BQ_SVC batched SMO solver whose columns are class pairs on an UNSORTED
 * panel, from the walkers' state on the device, after any run, finished or not: sklearn GridSearchCV's per-fold score of
 * OneVsOneClassifier(SVC(optimizer='smo')) (multiclass.py _ovr_decision_function and argmax on the fold's test rows), and no
 * columns x n array crosses the bus.  The sibling of bq_msolver_pairs_vote_heldout for bq_msmo.
 * ncls in [2, 64]; code: n class codes in [0, ncls); P = ncls (ncls - 1) / 2.  group_of / pair_of: k each, the group of a column in
 * [0, ngroups) and the number of its pair in the order (0,1), (0,2), ..., (1,2), ...; every group holds every pair exactly once, so
 * k = ngroups x P, ngroups in [1, 65535].  Every column carries a row list whose rows are of its pair's two classes, with label +1
 * on the larger class and -1 on the smaller (checked against the solver's host copy of its lists).  held: ngroups x n bytes, 1 a row
 * the group scores; such a row may be in no row list of its group.  A NULL argument (pred excepted), a BQ_SVR solver or anything
 * above that does not hold: BQ_ERR_BADARG, before any device call.
 * Per column: coef_i = a_i y_i where a_i > 1e-6, else 0; n_sv, the count of such rows; intercept = -(b_low + b_up) / 2 from the
 * column's record on the device, the bits of bq_msmo_get(BQ_SMO_SCALARS)[5]; u = K coef on all rows by the 16-column product, every
 * column in its own slot, in scratch of the call's own.
 * Per group: n_held, the held rows; every held row votes as bq_ovo_vote's rows do on u_k[row] + intercept_k over the group's P
 * columns in pair order; n_correct, the held rows whose predicted class is code[row]; a group with a column whose walker failed
 * reports n_correct = -1.  pred: NULL, or ngroups x n ints, the predicted class on the held rows and -1 elsewhere.  Integer sums in
 * a fixed order, no atomics: a group's results have the same bits alone, at any position and in any batch.  The solver's state and
 * liveness are untouched: a later run continues as without the call. */
int bq_msmo_vote_heldout(bq_msmo *s, int ncls, const int *code, int ngroups, const int *group_of, const int *pair_of,
                         const unsigned char *held, double *intercept, int64_t *n_sv, int64_t *n_held, int64_t *n_correct,
                         int *pred);
/* Held-out scores of the row-list columns of a batched SMO solver from the walkers' state on the device, after any run, finished
 * or not: the siblings of bq_msolver_svr_heldout / bq_msolver_svc_heldout for bq_msmo.  No k x n array crosses the bus, and the
 * solver's state and liveness are untouched: a later run continues as without the call.
 * held: nsets x n bytes, 1 on the rows a set scores (the test rows of a fold); set_of: k, the set whose rows column c scores, or -1:
 * no row.  A scoring column carries a row list, and none of its scored rows is in it.  BQ_ERR_BADARG before any device call: a NULL
 * argument (dec excepted), a solver of the other task, nsets < 1, an entry of set_of outside [-1, nsets) (of cal_of outside
 * [-1, ncal)), a problem without a resident panel, a scoring column without a list, a scored row in the column's own list.
 * Per column: coef_i = a_i y_i where a_i > 1e-6 (BQ_SVR: a+_i - a-_i where a+_i > 1e-6 or a-_i > 1e-6), else 0; n_sv, the count of
 * such rows; intercept from the column's record on the device, the bits of bq_msmo_get(BQ_SMO_SCALARS)[5] (-(b_low + b_up) / 2,
 * BQ_SVR: +(b_low + b_up) / 2); u = K coef on all rows by the 16-column product, every column in its own slot, in scratch of the
 * call's own.  A column whose walker failed reports NaN as its intercept (and sse, and decision values).
 * bq_msmo_svr_heldout: sse = sum (y_i - (u_i + intercept))^2 over the column's scored rows, y the column's targets as the solver
 * holds them, and n_held their count; a column without support vectors predicts its intercept (no NaN rule, unlike
 * bq_msolver_svr_heldout: SVR.fit's SMO branch divides by nothing).  One workgroup per column, sums in a fixed order, no atomics.
 * bq_msmo_svc_heldout: cal_of: k, column c's calibrator in [0, ncal) or -1; on the scored rows of a column with a calibrator the
 * decision value u_i + intercept and the label y_i (the solver's Y, which holds +-1 there) enter the calibrator's sample; columns
 * that share a calibrator score disjoint rows (else BQ_ERR_BADARG).  A, B, iters, loss, n_pos, n_neg, flags (ncal each) and dec
 * (NULL, or ncal x n: the decision values, 0 on the rows outside the sample) are bq_msolver_svc_heldout's.
 * Every figure of a column has the same bits alone, at any position and in any batch. */
int bq_msmo_svr_heldout(bq_msmo *s, int nsets, const int *set_of, const unsigned char *held, double *intercept, int64_t *n_sv,
                        double *sse, int64_t *n_held);
int bq_msmo_svc_heldout(bq_msmo *s, int nsets, const int *set_of, const unsigned char *held, int ncal, const int *cal_of,
                        double *intercept, int64_t *n_sv, double *A, double *B, int *iters, double *loss, int64_t *n_pos,
                        int64_t *n_neg, int *flags, double *dec);

/* ---- panel-free SMO: libsvm's WSS2 decomposition on kernel rows made on demand (bq_rsmo.hip) ---------------------------------
 * libsvm's Solver::Solve without shrinking (svm.cpp; the scalar rules are csrc/bq_rsmo_step.h, the NumPy restatement
 * tests/smo_rows_reference.py) on  min 1/2 a'Qa + p'a, y'a = 0, 0 <= a_t <= C_t:
 *   BQ_SVC  Q = diag(y) K diag(y), p = -1;   BQ_SVR  2n variables, Q = [[K, -K], [-K, K]], p = [epsilon - y; epsilon + y], signs
 *   [+1 ..; -1 ..], variables t and t + n share kernel row t.
 * Start alpha = 0, G = p; second-order working-set selection with TAU = 1e-12, ties to the LARGER index; stop when
 * Gmax + Gmax2 < tol — libsvm's (sklearn's) tol, not the two-threshold tol of bq_smo_create; rho = calculate_rho, intercept = -rho;
 * iteration cap max(10^7, 100 N) (test hook rsmo_max_steps).  No fused multiply-add on the path: the trajectory has the bits of the
 * restatement run on the rows bq_rsmo_rows returns.
 * p: a kernel-built BQ_STREAM problem on a single-rank context (anything else: BQ_ERR_BADARG before any device call); only its
 *    k-major image of X is read, one pass per kernel row.
 * task BQ_SVC: y in {+1,-1}, both present; BQ_SVR: targets.  Cw: n boxes, finite and > 0 (SVR: the box of both halves).
 * cache_rows: >= 2, or 0 = as many as fit the library's share (half) of the free device memory, at most n.  Rows live in an LRU
 *    cache managed on the device; a row has the same bits whenever it is computed, so nothing in a run depends on cache_rows.
 * bq_rsmo_run enqueues max_steps steps of two launches each with no host synchronisation in between, then reads the control
 *    block: *steps = pair updates done so far, *finished = 0 (running), 1 (optimal) or 2 (stopped at the cap).  Launches behind
 *    the step that finished return at once.  However a run is cut into calls, the iterates are the same.
 * bq_rsmo_rows: m x n kernel rows as the solver sees them (through the cache; each request counts as a hit or a miss). */
typedef struct bq_rsmo bq_rsmo;
enum { BQ_RSMO_ALPHAS = 0,    /* n (BQ_SVC) or [alpha; alpha*] 2n (BQ_SVR) */
       BQ_RSMO_GRADIENT = 1,  /* n | 2n */
       BQ_RSMO_SCALARS = 2,   /* 6: rho, Gmax, Gmax2 (of the last selection), last i, last j (of the last update; -1: none), steps */
       BQ_RSMO_STATS = 3,     /* 3: cache hits, misses, cache_rows */
       BQ_RSMO_NU_SCALARS = 4 /* 7, BQ_RSMO_RULE_NU only: rho, r, Gmaxp + Gmaxp2, Gmaxn + Gmaxn2, last i, last j, steps */ };
int bq_rsmo_create(bq_problem *p, int task, const double *y, const double *Cw, double epsilon, double tol,
                   int64_t cache_rows, bq_rsmo **out);
/* The general dual  min 1/2 a'Qa + lin'a,  0 <= a_v <= boxes_v,  Q_uv = s_u s_v K_row(u) row(v), from a start alpha0:
 *   BQ_RSMO_RULE_PLAIN  one equality s'a = s'alpha0: libsvm's Solver (bq_rsmo_create is this entry with alpha0 = 0 and its task's signs
 *                       and linear term; the one-class dual is signs +1, lin 0, boxes 1 and libsvm's start).
 *   BQ_RSMO_RULE_NU     the mass of each sign is kept: libsvm's Solver_NU (nu-SVC, nu-SVR) — one maximal violator per sign (ip over
 *                       s = +1 with a < C on -G, in over s = -1 with a > 0 on G), j scored against the row of its own sign, i = ip
 *                       or in according to s_j, stop when max(Gmaxp + Gmaxp2, Gmaxn + Gmaxn2) < tol, offsets r1 / r2 per sign with
 *                       rho = (r1 - r2) / 2 and r = (r1 + r2) / 2.  A step holds three rows: cache_rows 0 or >= 3.
 * N = n, or 2n with signs [+1 ..; -1 ..], the variables t and t + n sharing kernel row t.  max_steps: the iteration cap, 0 = libsvm's
 * max(10^7, 100 N); the hook rsmo_max_steps overrides either.
 * The start gradient is G0 = lin + s o (K b), b_t the sum of s_v alpha0_v over the variables of row t: lin's bits and no product
 * when b = 0, else ONE streamed Gram product of p (the product of bq_problem_matvec).  libsvm sums alpha_i Q_i in ascending i; G0
 * differs from that in rounding only.  G0 is computed once and depends neither on the cache nor on how the run is cut.
 * BQ_ERR_BADARG: what bq_rsmo_create refuses, alpha0 outside its box, a non-finite lin, signs other than +-1 (2n: other than
 * [+1 ..; -1 ..]), BQ_RSMO_RULE_NU with cache_rows 2 or with one sign only.
 * BQ_RSMO_SCALARS of a BQ_RSMO_RULE_NU solver: the same rho, then Gmaxp, Gmaxp2. */
enum { BQ_RSMO_RULE_PLAIN = 0, BQ_RSMO_RULE_NU = 1 };
int bq_rsmo_create_general(bq_problem *p, int rule, int64_t N, const double *signs, const double *lin, const double *boxes,
                           const double *alpha0, double tol, int64_t max_steps, int64_t cache_rows, bq_rsmo **out);
int bq_rsmo_run(bq_rsmo *s, int64_t max_steps, int64_t *steps, int *finished);
int bq_rsmo_get(bq_rsmo *s, int what, double *out);
int bq_rsmo_rows(bq_rsmo *s, int m, const int64_t *idx, double *out);
int bq_rsmo_destroy(bq_rsmo *s);

/* ---- prediction (optiml/ml/svm/_base.py:284-287) ------------------------------- */
/* out[t] = sum_m coef[m] * kernel(SV[m], Xt[t]) + intercept   (SV: m x d, Xt: t x d, row-major fp64) */
int bq_decision_function(bq_ctx *ctx, int kernel, double gamma, double coef0, int degree, int64_t m,
                         int64_t d, const double *SV, const double *coef, double intercept, int64_t t,
                         const double *Xt, double *out);

/* OUT (k x t, row-major) = W (k x m) . kernel(SV, Xt) + b; b == NULL: no intercepts.  One pass over the kernel values
   for all k columns; nothing of size t x m is held.  Row c's bits depend on W[c] and b[c] alone, not on k, on the other
   columns or on c's place among them.  BQ_ERR_BADARG for BQ_KERNEL_LAPLACIAN (no GEMM form). */
int bq_decision_function_multi(bq_ctx *ctx, int kernel, double gamma, double coef0, int degree, int64_t m, int64_t d,
                               const double *SV, int k, const double *W, const double *b, int64_t t, const double *Xt,
                               double *out);

/* ---- pairwise coupling (libsvm svm.cpp multiclass_probability: Wu, Lin & Weng 2004, second method; what
 * sklearn.svm.SVC(probability=True).predict_proba evaluates) ----------------------------------------------------------------------
 * ncls classes, P = ncls (ncls - 1) / 2 pair columns in the order (0,1), (0,2), ..., (1,2), ...; column q = (a, b), a < b, has class b
 * positive: s = 1 / (1 + exp(f A[q] + B[q])), evaluated without overflow and clipped to [1e-7, 1 - 1e-7], is the probability of b
 * against a (r[b][a] = s, r[a][b] = 1 - s).  Per test point p starts at 1 / ncls and takes libsvm's Gauss-Seidel sweeps until
 * max_t |(Qp)_t - p'Qp| < 0.005 / ncls, at most max(100, ncls) of them, one wavefront per point: no fused multiply-add, every sum
 * sequential in ascending index, IEEE division, so the same statements in NumPy on the same s give the same bits and sweep count.
 * A point's result has the same bits alone, at any position and in any batch.
 * F: t x P decision values (row-major, host); A, B: P; prob: t x ncls; iters: t sweeps taken (the cap when it was reached), or NULL;
 * R: t x P, the clipped s, or NULL.  ncls < 2, ncls > 64, t < 1 or a NULL required pointer: BQ_ERR_BADARG, before any device call. */
int bq_pairwise_coupling(bq_ctx *ctx, int ncls, int64_t t, const double *F, const double *A, const double *B, double *prob,
                         int *iters, double *R);
/* bq_decision_function_multi with k = P pair columns, and the coupling of each test point's P decision values where they lie on the
 * device, chunk of test points by chunk: prob, iters, R as above; dec: NULL, or k x t, which receives bq_decision_function_multi's
 * out (the same bits).  The checks are those of both; BQ_ERR_BADARG for BQ_KERNEL_LAPLACIAN and for k != ncls (ncls - 1) / 2. */
int bq_decision_coupled(bq_ctx *ctx, int kernel, double gamma, double coef0, int degree, int64_t m, int64_t d, const double *SV,
                        int k, const double *W, const double *b, int64_t t, const double *Xt, int ncls, const double *A,
                        const double *B, double *prob, int *iters, double *R, double *dec);

/* dense Gram matrix out (m x t, row-major) = kernel(A (m x d), B (t x d)); B == NULL means B is A (t ignored)
 * — the kernel functors' __call__, optiml/ml/svm/kernels.py:49-51 / 91-95 / 125-129 */
int bq_gram_matrix(bq_ctx *ctx, int kernel, double gamma, double coef0, int degree, int64_t m, int64_t d,
                   const double *A, int64_t t, const double *B, double *out);

/* x = A^-1 b for a dense symmetric positive definite A (n x n row-major fp64, lower triangle read):
 * scipy.linalg.cho_solve(cho_factor(A), b) at optiml/opti/constrained/interior_point.py:235 and
 * active_set.py:141.  BQ_ERR_NOT_PD mirrors LinAlgError.  factor_ms (optional): HIP-event time of the
 * factorisation alone. */
int bq_cholesky_solve(bq_ctx *ctx, int64_t n, const double *A, const double *b, double *x, double *factor_ms);

/* DIAGNOSTIC ENTRY: the factor and the solves of bq_cholesky_solve's kernels, as the solvers use them.  A (n x n row-major, lower
 * triangle read) is factored once; if sweeps != 0 the fast sweeps are prepared; then row j of B (nrhs x n, one right-hand side per
 * row) is solved as a right-hand side that vanishes before entry first_nonzero[j] (nrhs entries, or NULL for zeros) and the solution
 * arrives in row j of X (nrhs x n) through the solve's second output, the path ActiveSet takes.  L: NULL, or n x n, which receives
 * the lower triangle of the factor with zeros above it.  info: LAPACK's potrf value, 0 or 1 + the index of the first rejected
 * pivot; a non-zero info returns BQ_OK and leaves X and L untouched.  An entry of first_nonzero outside [0, n), or a row of B with
 * a non-zero before its entry: BQ_ERR_BADARG. */
int bq_cholesky_probe(bq_ctx *ctx, int64_t n, const double *A, int nrhs, const double *B, const int64_t *first_nonzero, int sweeps,
                      double *X, double *L, int *info);

#ifdef __cplusplus
}
#endif
#endif /* BCQP_H */
