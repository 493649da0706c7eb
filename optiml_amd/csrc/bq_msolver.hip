// Batched ProjectedGradient / FrankWolfe on k SVC duals that share one Gram panel (one-vs-rest multi-class: class c has labels
// y_c = +-1 and Q_c = diag(y_c) (K + 1) diag(y_c)).  Each class is an ordinary bq_solver (x, g, d, Qd, bounds, scalar state, records)
// and its iteration is the single-class one (bq_vec.hip: pgfw_update_kernel, bq_epilogue.h); what is batched is the launches:
//   update   (n/256 x k blocks)  the pending step and the new direction of every live class, W[:, pos[c]] = y_c o d_c
//   product  bq_launch_symm: one panel stream per chunk of BQ_SYMM_CK live classes
//   closing  (n/256 x k blocks)  Qd_c = y_c o OUT[:, pos[c]] and every class's sums and decisions (bq_epi_finish, per-class ticket)
//   live     (one wave)  the classes still running, in class order -> pos[], *nlive
// A class that stops leaves the product at the next iteration (its slot goes to the next live class); when none is left every
// kernel returns at once and the host stops enqueueing at its next lagged look at *nlive (bq_solver_run's polling scheme).
// Column c of the product has the same bits for any batch (bq_symm.hip), so every class follows the same trajectory in any batch.
//
// bq_msolver_create_boxes is the same solver with one box per column (UB: k x n, lb = 0) and the wide product (bq_symmw.hip, 16
// columns per panel stream) for every pass: the columns of a cross-validated search, (fold, C, class) with ub = C on the fold's
// training rows and 0 on its held-out rows.  A zero-width box keeps x = 0 there: the mid-box start is 0, PG zeroes d where
// ub - x <= ACT_TOL and x - lb <= ACT_TOL, FW's vertex is y = ub = lb = 0, so d = 0 and every sum of the column is its training
// fold's.
//
// bq_msolver_create_pairs is the boxes solver on a class-sorted panel with one column per one-vs-one pair (a, b): ub = C on the rows
// of a and b, 0 elsewhere, and the pair-routed product (bq_symmp.hip) for every pass, which streams the panel once for all pairs.
// The live kernel is the plan's: it keeps pos[] the identity (column = pair) and gathers every class's live pairs into the slots of
// its diagonal block; a stopped pair's blocks leave the stream at the next iteration.  bq_msolver_pairs_heldout scores its columns as
// bq_msolver_svc_heldout scores a boxes solver's (the folds of a one-vs-one calibration: ub = 0 on a fold's held-out rows of the pair's
// classes), with one routed product in which every pair is live.
//
// bq_msolver_create_svr is the same batch on a BQ_SVR problem (multi-output regression: target c has the linear term
// q_c = [-y_c; y_c] + eps and every target the Hessian [P -P; -P P]): the columns are vectors of 2n, one thread of the start-up and
// update kernels owns the elements i and n + i of a target (mstart_*_svr_kernel, mpgfw_update_svr_kernel), the product input is
// d+ - d- (n), and the closing kernel is mfinish_kernel, whose element code handles both halves (bq_epi_element).
//
// bq_msolver_create_al is the batch of k augmented-Lagrangian solvers (bq_al.hip; one-vs-rest SVC and multi-output SVR with the
// first-order rules: the unregularised intercept's equality row, the squared losses).  Column c is the bq_solver that
// bq_al_solver_create makes, with its own labels (BQ_SVC) or linear term (BQ_SVR); an iteration of all live columns is
//   [prep    (n/256 x k blocks)  BQ_SVR only: W[:, pos[c]] = x+ - x-, as the single solver's own launch for it]
//   product  bq_launch_symm, as above
//   closing  (n/256 x k blocks)  mal_finish_kernel: finish_al_kernel per column (bq_al_epi_*, the column's own ticket and partials)
//   live     mlive_kernel, BEFORE the update: the closing kernel is the one that stops a column, and the update writes the next
//            product's input, so it must see the slots of the next product
//   update   (N/256 x k blocks)  mal_update_kernel: al_update_body per column (bq_al_update.h), W[:, pos[c]] = y_c o x_new (BQ_SVC)
// A bq_msolver_run starts with the prep kernel (the flush of the run before may have stopped a column and moved the slots) and ends
// with mal_flush_kernel (al_flush_kernel per column) and the live kernel: a column's bits do not depend on how the iterations are
// cut into runs.  Nesterov momentum (a jump kernel and a flush per iteration) and schedules are not batched.
//
// bq_msolver_create_simplex is the batch of k nu-one-class duals on a BQ_PLAIN problem (bq_simplex.hip: the capped simplex
// {0 <= x <= UB[c], sum x = mass[c]} per column, spectral projected gradient).  Column c keeps its vectors, scalars and records in a
// bq_solver as the others do (x, g, d, ub, sc, stats), its step state in a bq_sx_state; an iteration of all live columns is
//   top      sx_top_kernel: the record and the stop tests of every live column, then mlive_kernel's numbering — BEFORE the projection,
//            which writes the product's input to the slots of this iteration's product
//   project  sx_project_kernel (one workgroup per column), product  bq_launch_symmw, close  sx_close_kernel
// so a run of max_steps iterations writes at most max_steps records per column, and a column's state after its last close waits
// for the next run's top.
#include "bq_al.h"
#include "bq_al_update.h"
#include "bq_common.h"
#include "bq_epilogue.h"
#include "bq_simplex.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

struct bq_msolver {
    bq_problem *p = nullptr;
    int kind = BQ_PG, k = 0;
    bool wide = false;   // bq_msolver_create_boxes / _svr_boxes: the 16-column product (bq_symmw.hip) for every pass
    bool svr_boxes = false;   // bq_msolver_create_svr_boxes: bq_msolver_svr_heldout may score it
    bool svc_boxes = false;   // bq_msolver_create_boxes: bq_msolver_svc_heldout may calibrate it
    // svc_boxes: k x n, 1 where UB is 0 (the column's held-out rows), as given at creation; a bq_msolver_create_pairs solver: the
    // same on the rows of the pair's classes and 0 on every other row (bq_msolver_pairs_heldout)
    std::vector<unsigned char> held;
    bq_pairs_plan *plan = nullptr;   // bq_msolver_create_pairs: the pair-routed product (bq_symmp.hip) for every pass
    int64_t ldw = 0;   // column stride of W / OUT / sgn (= p->ld >= nb * 256)
    std::vector<bq_solver *> cls;
    double *ql = nullptr;   // bq_msolver_create_svr: k x p->ldN, the linear term of every column (else every column has p->q)
    double *sgn = nullptr, *W = nullptr, *out = nullptr, *slab = nullptr;
    bq_epilogue *epi = nullptr;   // 2 x k: do_update 0 (a class's first iteration) and 1
    bq_scal **scs = nullptr;      // k
    int *pos = nullptr, *nlive = nullptr;
    int *nlive_host = nullptr;    // pinned copy of *nlive + its event (lagged polling)
    hipEvent_t flag_event = nullptr;
    int live_host = 0;            // upper bound of *nlive known to the host
    bool al = false;              // bq_msolver_create_al: the columns are augmented-Lagrangian solvers (epi: k entries of kind 2)
    bq_al_params al_prm = {};
    bool simplex = false;         // bq_msolver_create_simplex: the columns are capped-simplex solvers (bq_simplex.hip)
    bq_sx_col *sx_cols = nullptr;       // k: the device table of the columns
    bq_sx_state *sx_state = nullptr;    // k
    double *sx_rho = nullptr;           // k: bq_msolver_simplex_offsets' results on the device
    long long *sx_counts = nullptr;     // 2 k: its support and free counts
    std::vector<double> sx_mass;
    std::vector<int> sx_full;
    bool sx_has_x0 = false;
    struct bq_al_col *al_cols = nullptr;   // k: what mal_update_kernel reads of a column
    bool initialised = false, started = false;
};

__global__ __launch_bounds__(256) void mstart_prep_kernel(const bq_epilogue *__restrict__ epi, double *__restrict__ W, int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < e.n) W[blockIdx.y * ldw + i] = e.sgn[i] * e.x[i];
}

// prep_kernel + finish_kernel + grad_init_kernel of bq_pgfw_start, per class: Qd = y o (P (y o x)) (+ diag_add x), g = Qd + q
__global__ __launch_bounds__(256) void mstart_finish_kernel(const bq_epilogue *__restrict__ epi, const double *__restrict__ out, int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= e.N) return;
    double r = e.sgn[i] * out[blockIdx.y * ldw + i];
    if (e.diag_add != 0.0) r += e.diag_add * e.x[i];
    e.Qd[i] = r;
    e.g[i] = r + e.q[i];
}

// pgfw_update_kernel (bq_vec.hip) for BQ_SVC, class blockIdx.y, writing its product input to its slot
__global__ __launch_bounds__(256) void mpgfw_update_kernel(const bq_epilogue *__restrict__ epi, const int *__restrict__ pos,
                                                           double *__restrict__ W, int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    if (e.sc->done) return;
    double t, tr;
    bq_epi_scalars(e, t, tr);
    const bool upd = e.do_update != 0;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= e.n) return;
    const bq_pgfw_elem a = bq_pgfw_compute(e.kind, bq_pgfw_load(e, i, upd), upd, t, tr);
    if (upd) {
        e.x[i] = a.x;
        e.g[i] = a.g;
    }
    e.d[i] = a.d;
    W[pos[blockIdx.y] * ldw + i] = e.sgn[i] * a.d;
}

// mstart_prep_kernel for BQ_SVR: W[:, c] = x+ - x-
__global__ __launch_bounds__(256) void mstart_prep_svr_kernel(const bq_epilogue *__restrict__ epi, double *__restrict__ W, int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < e.n) W[blockIdx.y * ldw + i] = e.x[i] - e.x[e.n + i];
}

// mstart_finish_kernel for BQ_SVR, both halves of panel column i: Qd = [u; -u] (+ diag_add x), g = Qd + q_c, u = P (x+ - x-)
__global__ __launch_bounds__(256) void mstart_finish_svr_kernel(const bq_epilogue *__restrict__ epi, const double *__restrict__ out,
                                                                int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= e.n) return;
    const long long j = e.n + i;
    const double u = out[blockIdx.y * ldw + i], q0 = e.q[i], q1 = e.q[j];
    double r0 = u, r1 = -u;
    if (e.diag_add != 0.0) {
        r0 += e.diag_add * e.x[i];
        r1 += e.diag_add * e.x[j];
    }
    e.Qd[i] = r0;
    e.Qd[j] = r1;
    e.g[i] = r0 + q0;
    e.g[j] = r1 + q1;
}

// pgfw_update_kernel (bq_vec.hip) for BQ_SVR, target blockIdx.y: the elements i and n + i of one thread, both loaded before the
// first use, and the product input d+ - d- to the target's slot
__global__ __launch_bounds__(256) void mpgfw_update_svr_kernel(const bq_epilogue *__restrict__ epi, const int *__restrict__ pos,
                                                               double *__restrict__ W, int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    if (e.sc->done) return;
    double t, tr;
    bq_epi_scalars(e, t, tr);
    const bool upd = e.do_update != 0;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= e.n) return;
    const long long j = e.n + i;
    const bq_pgfw_raw r0 = bq_pgfw_load(e, i, upd), r1 = bq_pgfw_load(e, j, upd);
    const bq_pgfw_elem a = bq_pgfw_compute(e.kind, r0, upd, t, tr), b = bq_pgfw_compute(e.kind, r1, upd, t, tr);
    if (upd) {
        e.x[i] = a.x;
        e.g[i] = a.g;
        e.x[j] = b.x;
        e.g[j] = b.g;
    }
    e.d[i] = a.d;
    e.d[j] = b.d;
    W[pos[blockIdx.y] * ldw + i] = a.d - b.d;
}

// finish_den_kernel (bq_vec.hip) for class blockIdx.y: the same rows per block, the same tree, the class's own ticket
__global__ __launch_bounds__(256) void mfinish_kernel(const bq_epilogue *__restrict__ epi, const int *__restrict__ pos,
                                                      const double *__restrict__ out, int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    if (e.sc->done) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bq_epi_pre pre = bq_epi_preload(e, i, true);
    const double sv = i < e.n ? out[pos[blockIdx.y] * ldw + i] : 0.0;
    bq_epi_finish(e, blockIdx.x, gridDim.x, bq_epi_element(e, pre, i, sv), gridDim.x);
}

// bq_msolver_svr_heldout, column blockIdx.y: the coefficients of fitted_svr (svm/_batched.py), its threshold and its expression, to the
// column's own slot (not pos[]: every column is scored, live or not)
__global__ __launch_bounds__(256) void msvr_coef_kernel(const bq_epilogue *__restrict__ epi, double *__restrict__ W, int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= e.n) return;
    const double xp = e.x[i], xn = e.x[e.n + i];
    W[blockIdx.y * ldw + i] = (xp > 1e-6 || xn > 1e-6) ? xp - xn : 0.0;
}

// the fixed tree over the workgroup's 1024 partial sums and counts; every thread returns with the totals in s[0], c[0]
__device__ inline void msvr_tree(double *s, int *c, int tid) {
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if (tid < st) {
            s[tid] += s[tid + st];
            c[tid] += c[tid + st];
        }
        __syncthreads();
    }
}

// bq_msolver_svr_heldout, column blockIdx.x, u = out[:, column] = K coef.  Pass 1, the support rows (x+ or x- above 1e-6):
// S = sum (y - u), n_sv, b = (S - epsilon) / n_sv in svr_intercept's order.  Pass 2, the held-out rows (ub = 0 on both halves):
// sse = sum (y - (u + b))^2, n_held.  Thread t sums the rows t, t + 1024, ... in ascending order, then the tree: no atomics, and
// nothing of another column enters.  n_sv = 0: intercept = sse = NaN.
__global__ __launch_bounds__(1024) void msvr_score_kernel(const bq_epilogue *__restrict__ epi, const double *__restrict__ out, int64_t ldw,
                                                          const double *__restrict__ y, const double *__restrict__ epsilon,
                                                          double *__restrict__ intercept, long long *__restrict__ n_sv,
                                                          double *__restrict__ sse, long long *__restrict__ n_held) {
    __shared__ double sd[1024];
    __shared__ int sc[1024];
    const bq_epilogue &e = epi[blockIdx.x];
    const double *u = out + blockIdx.x * ldw;
    const int tid = threadIdx.x;
    const long long n = e.n;
    double s = 0.0;
    int cnt = 0;
    for (long long i = tid; i < n; i += 1024) {
        const bool sv = e.x[i] > 1e-6 || e.x[n + i] > 1e-6;
        s += sv ? y[i] - u[i] : 0.0;
        cnt += sv ? 1 : 0;
    }
    sd[tid] = s;
    sc[tid] = cnt;
    msvr_tree(sd, sc, tid);
    const int nsv = sc[0];
    double b = sd[0];
    b -= epsilon[blockIdx.x];
    b = nsv > 0 ? b / (double)nsv : NAN;
    __syncthreads();   // sd[0], sc[0] are read: pass 2 may overwrite them
    s = 0.0;
    cnt = 0;
    for (long long i = tid; i < n; i += 1024) {
        const bool held = e.ub[i] == 0.0 && e.ub[n + i] == 0.0;
        const double r = y[i] - (u[i] + b);
        s += held ? r * r : 0.0;
        cnt += held ? 1 : 0;
    }
    sd[tid] = s;
    sc[tid] = cnt;
    msvr_tree(sd, sc, tid);
    if (tid == 0) {
        intercept[blockIdx.x] = b;
        n_sv[blockIdx.x] = nsv;
        sse[blockIdx.x] = sd[0];   // NaN with b
        n_held[blockIdx.x] = sc[0];
    }
}

// bq_msolver_svc_heldout, column blockIdx.y: the coefficients of fitted_svc (svm/_batched.py), its threshold and its expression, to the
// column's own slot (not pos[]: every column is scored, live or not)
__global__ __launch_bounds__(256) void msvc_coef_kernel(const bq_epilogue *__restrict__ epi, double *__restrict__ W, int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= e.n) return;
    const double x = e.x[i];
    W[blockIdx.y * ldw + i] = x > 1e-6 ? x * e.sgn[i] : 0.0;
}

// the first pass of the held-out kernels of an SVC column, u = K coef: over the support rows (x above 1e-6) S = sum (y - u) and
// n_sv, summed as msvr_score_kernel sums; returns b = S / n_sv in intercept()'s order (svm/_batched.py; n_sv = 0: NaN) to every
// thread and writes both figures
__device__ inline double msvc_intercept(const bq_epilogue &e, const double *__restrict__ u, double *sd, int *sc, int tid,
                                        double *__restrict__ intercept, long long *__restrict__ n_sv) {
    const long long n = e.n;
    double s = 0.0;
    int cnt = 0;
    for (long long i = tid; i < n; i += 1024) {
        const bool sv = e.x[i] > 1e-6;
        s += sv ? e.sgn[i] - u[i] : 0.0;
        cnt += sv ? 1 : 0;
    }
    sd[tid] = s;
    sc[tid] = cnt;
    msvr_tree(sd, sc, tid);
    const int nsv = sc[0];
    const double b = nsv > 0 ? sd[0] / (double)nsv : NAN;
    if (tid == 0) {
        *intercept = b;
        *n_sv = nsv;
    }
    return b;
}

// bq_msolver_svc_heldout, column blockIdx.x, u = out[:, column] = K coef.  Pass 1: msvc_intercept.  Pass 2, the held-out rows
// (ub = 0): the decision value u + b and the label y to row cal_of[column] of D and L (row stride n; zeroed by the caller; the
// columns of a calibrator hold out disjoint rows, so no two workgroups write one entry).  n_sv = 0: b = NaN.
__global__ __launch_bounds__(1024) void msvc_heldout_kernel(const bq_epilogue *__restrict__ epi, const double *__restrict__ out,
                                                            int64_t ldw, const int *__restrict__ cal_of, double *__restrict__ D,
                                                            double *__restrict__ L, double *__restrict__ intercept,
                                                            long long *__restrict__ n_sv) {
    __shared__ double sd[1024];
    __shared__ int sc[1024];
    const bq_epilogue &e = epi[blockIdx.x];
    const double *u = out + blockIdx.x * ldw;
    const int tid = threadIdx.x;
    const long long n = e.n;
    const double b = msvc_intercept(e, u, sd, sc, tid, intercept + blockIdx.x, n_sv + blockIdx.x);
    const int cal = cal_of[blockIdx.x];
    if (cal < 0) return;
    double *d = D + (long long)cal * n, *l = L + (long long)cal * n;
    for (long long i = tid; i < n; i += 1024) {
        if (e.ub[i] == 0.0) {
            d[i] = u[i] + b;
            l[i] = e.sgn[i];
        }
    }
}

// bq_msolver_pairs_heldout, column blockIdx.x = pair (a, b) of a class-sorted panel: msvc_heldout_kernel, whose held-out rows are
// the data rows (data_row: 1; a ghost row: 0) of the tile rows of a and of b with ub = 0 — ub is 0 on every row of another class
// too, and such a row is in no pair's sample
__global__ __launch_bounds__(1024) void mpairs_heldout_kernel(const bq_epilogue *__restrict__ epi, const double *__restrict__ out,
                                                              int64_t ldw, const int *__restrict__ pairs, const int *__restrict__ ct,
                                                              const unsigned char *__restrict__ data_row,
                                                              const int *__restrict__ cal_of, double *__restrict__ D,
                                                              double *__restrict__ L, double *__restrict__ intercept,
                                                              long long *__restrict__ n_sv) {
    __shared__ double sd[1024];
    __shared__ int sc[1024];
    const bq_epilogue &e = epi[blockIdx.x];
    const double *u = out + blockIdx.x * ldw;
    const int tid = threadIdx.x;
    const long long n = e.n;
    const double b = msvc_intercept(e, u, sd, sc, tid, intercept + blockIdx.x, n_sv + blockIdx.x);
    const int cal = cal_of[blockIdx.x];
    if (cal < 0) return;
    double *d = D + (long long)cal * n, *l = L + (long long)cal * n;
    for (int side = 0; side < 2; ++side) {
        const int cls = pairs[2 * blockIdx.x + side];
        const long long r1 = (long long)ct[cls + 1] * BQ_SYM_TILE < n ? (long long)ct[cls + 1] * BQ_SYM_TILE : n;
        for (long long i = (long long)ct[cls] * BQ_SYM_TILE + tid; i < r1; i += 1024) {
            if (data_row[i] && e.ub[i] == 0.0) {
                d[i] = u[i] + b;
                l[i] = e.sgn[i];
            }
        }
    }
}

// ---- the augmented-Lagrangian batch: what al_update_kernel takes as arguments, per column
struct bq_al_col {
    bq_al_vecs V;
    bq_scal *sc;
    const double *sgn;   // the column's labels (BQ_SVC), else null
};

// the product input of every live column from its point: y_c o x (BQ_SVC) or x+ - x- (BQ_SVR), to the column's slot
__global__ __launch_bounds__(256) void mal_prep_kernel(const bq_epilogue *__restrict__ epi, const int *__restrict__ pos,
                                                       double *__restrict__ W, int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    if (e.sc->done) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= e.n) return;
    W[pos[blockIdx.y] * ldw + i] = e.structure == BQ_SVR ? e.x[i] - e.x[e.n + i] : e.sgn[i] * e.x[i];
}

// finish_al_kernel (bq_al.hip) for column blockIdx.y: the same rows per block, the same tree, the column's own ticket and partials
__global__ __launch_bounds__(256) void mal_finish_kernel(const bq_epilogue *__restrict__ epi, const int *__restrict__ pos,
                                                         const double *__restrict__ out, int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    if (e.sc->done) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bq_al_pre pre = bq_al_epi_preload(e, i, true, true);
    const double sv = i < e.n ? out[pos[blockIdx.y] * ldw + i] : 0.0;
    bq_al_epi_finish<true>(e, blockIdx.x, gridDim.x, bq_al_epi_element(e, pre, i, sv, true), gridDim.x);
}

// al_flush_kernel (bq_al.hip) for column blockIdx.y
__global__ __launch_bounds__(256) void mal_flush_kernel(const bq_epilogue *__restrict__ epi) {
    const bq_epilogue &e = epi[blockIdx.y];
    if (e.sc->done || !e.sc->al_pending) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bq_al_pre pre = bq_al_epi_preload(e, i, true, false);
    bq_al_epi_finish<false>(e, blockIdx.x, gridDim.x, bq_al_epi_element(e, pre, i, 0.0, false), gridDim.x);
}

// al_update_kernel (bq_al.hip) for column blockIdx.y, writing the next product's input to the column's slot (BQ_SVC).  A column
// that the closing kernel has just stopped has a stale pos[] entry (< k): al_update_body writes no input for it
__global__ __launch_bounds__(256) void mal_update_kernel(int64_t N, int64_t ldN, const bq_al_col *__restrict__ cols, bq_al_params prm,
                                                         const int *__restrict__ pos, double *__restrict__ W, int64_t ldw) {
    const bq_al_col &c = cols[blockIdx.y];
    al_update_body(N, ldN, c.V, prm, c.sc, c.sgn, c.sgn != nullptr ? W + pos[blockIdx.y] * ldw : nullptr);
}

__global__ void mlive_kernel(bq_scal *const *__restrict__ scs, int k, int *__restrict__ pos, int *__restrict__ nlive) {
    if (threadIdx.x != 0) return;
    int s = 0;
    for (int c = 0; c < k; ++c)
        if (!scs[c]->done) pos[c] = s++;
    *nlive = s;
}

extern "C" int bq_msolver_destroy(bq_msolver *m) {
    if (m == nullptr) return BQ_OK;
    hipSetDevice(m->p->ctx->device);
    (void)bq_ctx_sync(m->p->ctx);
    for (void *ptr : {(void *)m->ql, (void *)m->sgn, (void *)m->W, (void *)m->out, (void *)m->slab, (void *)m->epi, (void *)m->scs, (void *)m->pos,
                      (void *)m->nlive, (void *)m->al_cols, (void *)m->sx_cols, (void *)m->sx_state, (void *)m->sx_rho, (void *)m->sx_counts})
        if (ptr) hipFree(ptr);
    if (m->nlive_host) {
        hipHostFree(m->nlive_host);
        hipEventDestroy(m->flag_event);
    }
    for (bq_solver *s : m->cls) bq_solver_destroy(s);
    bq_pairs_plan_destroy(m->plan);
    bq_problem *p = m->p;
    delete m;
    bq_problem_unref(p);
    return BQ_OK;
}

static void fill_epi(bq_msolver *m, int c, int do_update, bq_epilogue &e) {
    const bq_solver *s = m->cls[c];
    const bq_problem *p = m->p;
    e = bq_epilogue{};
    e.structure = p->structure;
    e.kind = m->kind == BQ_PG ? 0 : 1;
    e.do_update = do_update;
    e.n = p->n;
    e.N = p->N;
    e.diag_add = p->diag_add;
    e.x = s->x;
    e.g = s->g;
    e.d = s->d;
    e.q = m->ql ? m->ql + c * p->ldN : p->q;
    e.lb = s->lb;
    e.ub = s->ub;
    e.sgn = m->sgn ? m->sgn + c * m->ldw : nullptr;
    e.Qd = s->Qd;
    e.sc = s->sc;
    e.part = s->partials;
    e.stats = s->stats;
}

// the device epilogue table: the records' buffers may have been re-allocated by a run with more steps
static int upload_epi(bq_msolver *m) {
    if (m->simplex) {
        std::vector<bq_sx_col> h((size_t)m->k);
        for (int c = 0; c < m->k; ++c) {
            const bq_solver *s = m->cls[c];
            h[c] = bq_sx_col{(long long)m->p->n, s->x, s->g, s->d, s->ub, m->sx_mass[c], m->sx_full[c], m->sx_has_x0 ? 1 : 0,
                             s->sc, m->sx_state + c, s->stats};
        }
        BQ_HIP(hipMemcpyAsync(m->sx_cols, h.data(), sizeof(bq_sx_col) * h.size(), hipMemcpyHostToDevice, m->p->ctx->stream));
        BQ_SYNC(m->p->ctx);   // h goes out of scope
        return BQ_OK;
    }
    if (m->al) {
        std::vector<bq_epilogue> h((size_t)m->k);
        std::vector<bq_al_col> cols((size_t)m->k);
        for (int c = 0; c < m->k; ++c) {
            const double *sgn = m->sgn ? m->sgn + c * m->ldw : nullptr;
            h[c] = bq_al_epilogue(m->cls[c]);   // q: the column's own (V.q, bq_msolver_create_al)
            h[c].sgn = sgn;
            cols[c] = bq_al_col{m->cls[c]->al->V, m->cls[c]->sc, sgn};
        }
        BQ_HIP(hipMemcpyAsync(m->epi, h.data(), sizeof(bq_epilogue) * h.size(), hipMemcpyHostToDevice, m->p->ctx->stream));
        BQ_HIP(hipMemcpyAsync(m->al_cols, cols.data(), sizeof(bq_al_col) * cols.size(), hipMemcpyHostToDevice, m->p->ctx->stream));
        BQ_SYNC(m->p->ctx);   // h, cols go out of scope
        return BQ_OK;
    }
    std::vector<bq_epilogue> h(2 * (size_t)m->k);
    for (int c = 0; c < m->k; ++c) {
        fill_epi(m, c, 0, h[c]);
        fill_epi(m, c, 1, h[m->k + c]);
    }
    BQ_HIP(hipMemcpyAsync(m->epi, h.data(), sizeof(bq_epilogue) * h.size(), hipMemcpyHostToDevice, m->p->ctx->stream));
    BQ_SYNC(m->p->ctx);   // h goes out of scope
    return BQ_OK;
}

static int msolver_ck(const bq_msolver *m) { return m->wide ? BQ_SYMMW_CK : BQ_SYMM_CK; }

static int msolver_product(bq_msolver *m, int slots) {
    bq_problem *p = m->p;
    if (m->plan) return bq_launch_symmp(p, m->plan, p->add_one, m->W, m->ldw, m->slab, m->out);
    if (m->wide) return bq_launch_symmw(p, p->add_one, m->W, m->ldw, slots, m->slab, m->out, m->nlive);
    return bq_launch_symm(p, p->add_one, m->W, m->ldw, slots, m->slab, m->out, m->nlive);
}

// ub_ld: 0 (one box for every class) or n (class c's box at ub + c * n); plan: the pair-routed product (taken over by the solver);
// QL: null (a BQ_SVC problem, Y: k x n labels), or the k x 2n linear terms of a BQ_SVR problem (Y null)
static int msolver_create(bq_problem *p, int kind, int k, const double *Y, const double *ub, int64_t ub_ld, bool wide,
                          const double *x0, double eps, int64_t max_iter, double fw_t, bq_msolver **out,
                          bq_pairs_plan *plan = nullptr, const double *QL = nullptr);

static int msolver_check(bq_problem *p, int kind, int k, const double *Y, const double *ub, bq_msolver **out,
                         const double *QL = nullptr) {
    BQ_ARG(p && (Y || QL) && ub && out, "NULL argument");
    BQ_ARG(kind == BQ_PG || kind == BQ_FW, "the batched solver is ProjectedGradient or FrankWolfe");
    BQ_ARG(k >= 1, "k must be >= 1");
    if (QL)
        BQ_ARG(p->structure == BQ_SVR && p->kernel >= 0, "the batched SVR solver takes a kernel-built SVR problem");
    else
        BQ_ARG(p->structure == BQ_SVC && p->kernel >= 0, "the batched solver takes a kernel-built SVC problem");
    if (p->ctx->world != 1 || p->streamed || !p->symmetric) {
        bq_set_error("the batched solver needs a single-rank context and a resident packed panel (not streamed, not full rows)");
        return BQ_ERR_BADARG;
    }
    if (QL) {
        for (int64_t i = 0; i < (int64_t)k * p->N; ++i) BQ_ARG(std::isfinite(QL[i]), "the linear terms must be finite");
        return BQ_OK;
    }
    for (int64_t i = 0; i < (int64_t)k * p->n; ++i) BQ_ARG(Y[i] == 1.0 || Y[i] == -1.0, "labels must be +1 or -1");
    return BQ_OK;
}

// everything of a batched solver but its columns' solvers (m->cls, m->k, m->ldw, m->wide, m->plan are set): the per-column labels or
// linear terms (both null: none), the product's W / OUT / slab, the tables.  The caller destroys m on failure.
static int msolver_alloc(bq_msolver *m, const double *Y, const double *QL) {
    bq_problem *p = m->p;
    bq_ctx *c = p->ctx;
    const int k = m->k;
    const bool wide = m->wide;
    const bq_pairs_plan *plan = m->plan;
    const int slots = (int)bq_round_up(k, msolver_ck(m));
    // the per-column host array and its device copy: the labels (k x n -> sgn, stride ldw) or the linear terms (k x 2n -> ql, stride ldN)
    const double *col_src = QL ? QL : Y;
    double **col_dev = QL ? &m->ql : &m->sgn;
    const int64_t col_len = QL ? p->N : p->n, col_ld = QL ? p->ldN : m->ldw;
    hipError_t e = col_src ? hipMalloc(col_dev, sizeof(double) * col_ld * k) : hipSuccess;
    if (e == hipSuccess) e = hipMalloc(&m->W, sizeof(double) * m->ldw * slots);
    if (e == hipSuccess) e = hipMalloc(&m->out, sizeof(double) * m->ldw * slots);
    const int64_t slab_len = plan ? bq_pairs_slab_len(plan) : wide ? bq_symmw_slab_len(p->nb) : bq_symm_slab_len(p->nb);
    if (e == hipSuccess) e = hipMalloc(&m->slab, sizeof(double) * slab_len);
    if (e == hipSuccess) e = hipMalloc(&m->epi, sizeof(bq_epilogue) * 2 * k);
    if (e == hipSuccess && m->al) e = hipMalloc(&m->al_cols, sizeof(bq_al_col) * k);
    if (e == hipSuccess) e = hipMalloc(&m->scs, sizeof(bq_scal *) * k);
    if (e == hipSuccess) e = hipMalloc(&m->pos, sizeof(int) * k);
    if (e == hipSuccess) e = hipMalloc(&m->nlive, sizeof(int));
    if (e != hipSuccess) {
        bq_set_error("batched solver: device allocation failed: %s", hipGetErrorString(e));
        return BQ_ERR_NOMEM;
    }
    std::vector<bq_scal *> scs(k);
    std::vector<int> pos(k);
    for (int cl = 0; cl < k; ++cl) {
        scs[cl] = m->cls[cl]->sc;
        pos[cl] = cl;
    }
    hipStream_t st = c->stream;
    if (col_src) e = hipMemsetAsync(*col_dev, 0, sizeof(double) * col_ld * k, st);
    if (e == hipSuccess) e = hipMemsetAsync(m->W, 0, sizeof(double) * m->ldw * slots, st);
    if (e == hipSuccess) e = hipMemsetAsync(m->out, 0, sizeof(double) * m->ldw * slots, st);
    if (e == hipSuccess && col_src) e = hipMemcpy2DAsync(*col_dev, sizeof(double) * col_ld, col_src, sizeof(double) * col_len,
                                              sizeof(double) * col_len, k, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(m->scs, scs.data(), sizeof(bq_scal *) * k, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(m->pos, pos.data(), sizeof(int) * k, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(m->nlive, &k, sizeof(int), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) {
        bq_set_error("batched solver setup failed: %s", hipGetErrorString(e));
        return BQ_ERR_HIP;
    }
    if (hipHostMalloc((void **)&m->nlive_host, sizeof(int), hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&m->flag_event, hipEventDisableTiming) != hipSuccess) {
        if (m->nlive_host) hipHostFree(m->nlive_host);
        m->nlive_host = nullptr;
        (void)hipGetLastError();
    }
    m->live_host = k;
    return BQ_OK;
}

static int msolver_create(bq_problem *p, int kind, int k, const double *Y, const double *ub, int64_t ub_ld, bool wide,
                          const double *x0, double eps, int64_t max_iter, double fw_t, bq_msolver **out, bq_pairs_plan *plan,
                          const double *QL) {
    if (int rc = msolver_check(p, kind, k, Y, ub, out, QL)) {
        bq_pairs_plan_destroy(plan);
        return rc;
    }
    bq_ctx *c = p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    bq_msolver *m = new bq_msolver();
    m->p = p;
    p->refs += 1;
    m->kind = kind;
    m->k = k;
    m->ldw = p->ld;   // (= p->ldN for BQ_SVC)
    m->wide = wide;
    m->plan = plan;
    int rc = BQ_OK;
    for (int cl = 0; cl < k && rc == BQ_OK; ++cl) {
        bq_solver *s = nullptr;
        rc = bq_solver_create(p, kind, nullptr, ub + cl * ub_ld, x0 ? x0 + (int64_t)cl * p->N : nullptr, eps, max_iter, fw_t, &s);
        if (rc == BQ_OK) m->cls.push_back(s);
    }
    auto fail = [&](int code) {
        bq_msolver_destroy(m);
        return code;
    };
    if (rc != BQ_OK) return fail(rc);
    rc = msolver_alloc(m, Y, QL);
    if (rc != BQ_OK) return fail(rc);
    rc = upload_epi(m);
    if (rc != BQ_OK) return fail(rc);
    *out = m;
    return BQ_OK;
}

extern "C" int bq_msolver_create(bq_problem *p, int kind, int k, const double *Y, const double *ub, const double *x0, double eps,
                                 int64_t max_iter, double fw_t, bq_msolver **out) {
    return msolver_create(p, kind, k, Y, ub, 0, false, x0, eps, max_iter, fw_t, out);
}

extern "C" int bq_msolver_create_boxes(bq_problem *p, int kind, int k, const double *Y, const double *UB, const double *x0,
                                       double eps, int64_t max_iter, double fw_t, bq_msolver **out) {
    BQ_ARG(p && UB, "NULL argument");
    for (int64_t i = 0; i < (int64_t)k * p->n; ++i) BQ_ARG(UB[i] >= 0.0, "upper bounds must be >= 0 (lb = 0)");
    BQ_TRY(msolver_create(p, kind, k, Y, UB, p->n, true, x0, eps, max_iter, fw_t, out));
    bq_msolver *m = *out;
    try {
        m->held.resize((size_t)k * (size_t)p->n);
    } catch (const std::bad_alloc &) {   // no exception leaves the C ABI, and the solver does not outlive the failure
        bq_msolver_destroy(m);
        *out = nullptr;
        bq_set_error("batched solver: no host memory for the held-out masks");
        return BQ_ERR_NOMEM;
    }
    for (size_t i = 0; i < m->held.size(); ++i) m->held[i] = UB[i] == 0.0;
    m->svc_boxes = true;
    return BQ_OK;
}

extern "C" int bq_msolver_create_pairs(bq_problem *p, int kind, int ncls, const int *cls_tiles, int m, const int *pairs,
                                       const double *Y, const double *UB, const double *x0, double eps, int64_t max_iter, double fw_t,
                                       bq_msolver **out) {
    BQ_TRY(msolver_check(p, kind, m, Y, UB, out));
    BQ_HIP(hipSetDevice(p->ctx->device));
    bq_pairs_plan *plan = nullptr;
    BQ_TRY(bq_pairs_plan_create(p, ncls, cls_tiles, m, pairs, &plan));   // validates cls_tiles and pairs
    for (int q = 0; q < m; ++q) {
        const int64_t a0 = (int64_t)cls_tiles[pairs[2 * q]] * BQ_SYM_TILE, a1 = (int64_t)cls_tiles[pairs[2 * q] + 1] * BQ_SYM_TILE;
        const int64_t b0 = (int64_t)cls_tiles[pairs[2 * q + 1]] * BQ_SYM_TILE, b1 = (int64_t)cls_tiles[pairs[2 * q + 1] + 1] * BQ_SYM_TILE;
        for (int64_t i = 0; i < p->n; ++i) {
            const double u = UB[q * p->n + i];
            const bool mine = (i >= a0 && i < a1) || (i >= b0 && i < b1);
            if (!(u >= 0.0) || (!mine && u != 0.0)) {
                bq_pairs_plan_destroy(plan);
                bq_set_error("bad argument: upper bounds must be >= 0 on the pair's rows and 0 on every other row");
                return BQ_ERR_BADARG;
            }
        }
    }
    BQ_TRY(msolver_create(p, kind, m, Y, UB, p->n, false, x0, eps, max_iter, fw_t, out, plan));
    bq_msolver *s = *out;
    try {
        s->held.assign((size_t)m * (size_t)p->n, 0);
    } catch (const std::bad_alloc &) {   // as bq_msolver_create_boxes
        bq_msolver_destroy(s);
        *out = nullptr;
        bq_set_error("batched solver: no host memory for the held-out masks");
        return BQ_ERR_NOMEM;
    }
    for (int q = 0; q < m; ++q)
        for (int e = 0; e < 2; ++e) {
            const int64_t r0 = (int64_t)cls_tiles[pairs[2 * q + e]] * BQ_SYM_TILE;
            const int64_t r1 = std::min<int64_t>((int64_t)cls_tiles[pairs[2 * q + e] + 1] * BQ_SYM_TILE, p->n);
            for (int64_t i = r0; i < r1; ++i) s->held[(size_t)q * (size_t)p->n + i] = UB[q * p->n + i] == 0.0;
        }
    return BQ_OK;
}

extern "C" int bq_msolver_create_svr(bq_problem *p, int kind, int k, const double *QL, const double *ub, const double *x0,
                                     double eps, int64_t max_iter, double fw_t, bq_msolver **out) {
    return msolver_create(p, kind, k, nullptr, ub, 0, false, x0, eps, max_iter, fw_t, out, nullptr, QL);
}

extern "C" int bq_msolver_create_svr_boxes(bq_problem *p, int kind, int k, const double *QL, const double *UB, const double *x0,
                                           double eps, int64_t max_iter, double fw_t, bq_msolver **out) {
    BQ_ARG(p && UB && out, "NULL argument");
    BQ_ARG(k >= 1, "k must be >= 1");
    BQ_ARG(p->structure == BQ_SVR, "the batched SVR solver takes a kernel-built SVR problem");
    for (int c = 0; c < k; ++c) {
        const double *ub = UB + (int64_t)c * p->N;
        for (int64_t i = 0; i < p->N; ++i) BQ_ARG(ub[i] >= 0.0, "upper bounds must be >= 0 (lb = 0)");
        for (int64_t i = 0; i < p->n; ++i)
            BQ_ARG((ub[i] == 0.0) == (ub[p->n + i] == 0.0), "a held-out row has ub = 0 on both halves: one half alone is zero");
    }
    BQ_TRY(msolver_create(p, kind, k, nullptr, UB, p->N, true, x0, eps, max_iter, fw_t, out, nullptr, QL));
    (*out)->svr_boxes = true;
    return BQ_OK;
}

extern "C" int bq_msolver_create_al(bq_problem *p, const bq_al_params *prm, int k, const double *Y, const double *QL,
                                    const double *a_eq, int64_t a_ld, const double *lb, const double *ub, const double *x0,
                                    const double *dual0, bq_msolver **out) {
    BQ_ARG(p && prm && x0 && out, "NULL argument");
    BQ_ARG(k >= 1, "k must be >= 1");
    BQ_ARG(p->kernel >= 0 && (p->structure == BQ_SVC || p->structure == BQ_SVR),
           "the batched augmented-Lagrangian solver takes a kernel-built SVC or SVR problem");
    if (p->structure == BQ_SVC) BQ_ARG(Y != nullptr && QL == nullptr, "a BQ_SVC problem takes the labels Y and no linear terms");
    else BQ_ARG(Y == nullptr, "a BQ_SVR problem takes no labels");
    if (p->ctx->world != 1 || p->streamed || !p->symmetric) {
        bq_set_error("the batched solver needs a single-rank context and a resident packed panel (not streamed, not full rows)");
        return BQ_ERR_BADARG;
    }
    BQ_ARG(prm->momentum_type != BQ_MOM_NESTEROV, "Nesterov momentum is not batched: one bq_al_solver_create per column");
    BQ_ARG(a_eq == nullptr || a_ld == 0 || a_ld == p->N, "a_ld is 0 (one equality row for every column) or N (one per column)");
    if (Y)
        for (int64_t i = 0; i < (int64_t)k * p->n; ++i) BQ_ARG(Y[i] == 1.0 || Y[i] == -1.0, "labels must be +1 or -1");
    if (QL)
        for (int64_t i = 0; i < (int64_t)k * p->N; ++i) BQ_ARG(std::isfinite(QL[i]), "the linear terms must be finite");
    bq_ctx *c = p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    bq_msolver *m = new bq_msolver();
    m->p = p;
    p->refs += 1;
    m->al = true;
    m->al_prm = *prm;
    m->k = k;
    m->ldw = p->ld;
    const int64_t n_dual = (a_eq ? 1 : 0) + (lb ? p->N : 0) + (ub ? p->N : 0);
    int rc = BQ_OK;
    for (int cl = 0; cl < k && rc == BQ_OK; ++cl) {
        bq_solver *s = nullptr;   // the rule's parameters are checked here, as for a single solver
        rc = bq_al_solver_create(p, prm, a_eq ? a_eq + cl * a_ld : nullptr, lb, ub, x0 + (int64_t)cl * p->N,
                                 dual0 && n_dual > 0 ? dual0 + cl * n_dual : nullptr, &s);
        if (rc == BQ_OK) m->cls.push_back(s);
    }
    if (rc == BQ_OK) rc = msolver_alloc(m, Y, QL);
    if (rc == BQ_OK && m->ql)
        for (int cl = 0; cl < k; ++cl) m->cls[cl]->al->V.q = m->ql + cl * p->ldN;   // not the solver's to free (as p->q)
    if (rc == BQ_OK) rc = upload_epi(m);
    if (rc != BQ_OK) {
        bq_msolver_destroy(m);
        return rc;
    }
    m->initialised = true;   // no start-up product: every iteration evaluates Q x afresh
    *out = m;
    return BQ_OK;
}

extern "C" int bq_msolver_create_simplex(bq_problem *p, int k, const double *UB, const double *mass, const double *x0, double tol,
                                         int64_t max_iter, bq_msolver **out) {
    BQ_ARG(p && UB && mass && out, "NULL argument");
    BQ_ARG(k >= 1, "k must be >= 1");
    BQ_ARG(p->structure == BQ_PLAIN && p->kernel >= 0, "the simplex solver takes a kernel-built BQ_PLAIN problem");
    BQ_ARG(p->diag_add == 0.0, "the simplex solver takes a problem without a diagonal term");
    if (p->ctx->world != 1 || p->streamed || !p->symmetric) {
        bq_set_error("the batched solver needs a single-rank context and a resident packed panel (not streamed, not full rows)");
        return BQ_ERR_BADARG;
    }
    BQ_ARG(tol >= 0.0, "tol must be >= 0");
    const int64_t n = p->n;
    std::vector<int> full((size_t)k);
    BQ_TRY(bq_sx_check(k, n, UB, mass, full.data()));
    if (x0)   // inside its set: the box exactly, the mass to the rounding of a sum of n terms
        for (int c = 0; c < k; ++c) {
            long double sum = 0.0L;
            for (int64_t i = 0; i < n; ++i) {
                const double x = x0[(int64_t)c * n + i];
                BQ_ARG(x >= 0.0 && x <= UB[(int64_t)c * n + i], "x0 must lie in its box");
                sum += x;
            }
            BQ_ARG(std::fabs((double)sum - mass[c]) <= (double)n * 2.220446049250313e-16 * mass[c], "x0 must sum to its column's mass");
        }
    bq_ctx *c = p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    bq_msolver *m = new bq_msolver();
    m->p = p;
    p->refs += 1;
    m->kind = BQ_PG;
    m->k = k;
    m->ldw = p->ld;
    m->wide = true;
    m->simplex = true;
    m->sx_has_x0 = x0 != nullptr;
    m->sx_mass.assign(mass, mass + k);
    m->sx_full = full;
    const std::vector<double> zero(x0 ? 0 : (size_t)n, 0.0);
    int rc = BQ_OK;
    for (int cl = 0; cl < k && rc == BQ_OK; ++cl) {
        bq_solver *s = nullptr;   // the column's vectors, scalars (eps = tol) and records
        rc = bq_solver_create(p, BQ_PG, nullptr, UB + (int64_t)cl * n, x0 ? x0 + (int64_t)cl * n : zero.data(), tol, max_iter, 0.0, &s);
        if (rc == BQ_OK) m->cls.push_back(s);
    }
    if (rc == BQ_OK) rc = msolver_alloc(m, nullptr, nullptr);
    if (rc == BQ_OK) {
        hipError_t e = hipMalloc(&m->sx_cols, sizeof(bq_sx_col) * k);
        if (e == hipSuccess) e = hipMalloc(&m->sx_state, sizeof(bq_sx_state) * k);
        if (e == hipSuccess) e = hipMalloc(&m->sx_rho, sizeof(double) * k);
        if (e == hipSuccess) e = hipMalloc(&m->sx_counts, sizeof(long long) * 2 * k);
        if (e == hipSuccess) e = hipMemsetAsync(m->sx_state, 0, sizeof(bq_sx_state) * k, c->stream);
        if (e != hipSuccess) {
            bq_set_error("batched solver: device allocation failed: %s", hipGetErrorString(e));
            rc = BQ_ERR_NOMEM;
        }
    }
    if (rc == BQ_OK) rc = upload_epi(m);
    if (rc != BQ_OK) {
        bq_msolver_destroy(m);
        return rc;
    }
    *out = m;
    return BQ_OK;
}

extern "C" int bq_msolver_simplex_offsets(bq_msolver *m, double *rho, int64_t *n_sv, int64_t *n_free) {
    BQ_ARG(m && rho && n_sv && n_free, "NULL argument");
    BQ_ARG(m->simplex, "the offsets take a solver of bq_msolver_create_simplex");
    BQ_ARG(m->initialised, "the offsets take a solver that has run");
    bq_ctx *c = m->p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int k = m->k;
    double *dr = m->sx_rho;
    long long *dn = m->sx_counts;
    int rc = bq_sx_launch_offsets(m->sx_cols, k, dr, dn, dn + k, st);
    if (rc == BQ_OK) {
        static_assert(sizeof(long long) == sizeof(int64_t), "the counts are copied as int64_t");
        hipError_t e = hipMemcpyAsync(rho, dr, sizeof(double) * k, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(n_sv, dn, sizeof(int64_t) * k, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(n_free, dn + k, sizeof(int64_t) * k, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) {
            bq_set_error("simplex offsets: %s", hipGetErrorString(e));
            rc = BQ_ERR_HIP;
        }
    }
    if (rc == BQ_OK) rc = bq_ctx_sync(c);
    else (void)bq_ctx_sync(c);
    return rc;
}

extern "C" int bq_msolver_svr_heldout(bq_msolver *m, const double *y, const double *epsilon, double *intercept, int64_t *n_sv,
                                      double *sse, int64_t *n_held) {
    BQ_ARG(m && y && epsilon && intercept && n_sv && sse && n_held, "NULL argument");
    BQ_ARG(m->svr_boxes, "held-out scoring takes a solver of bq_msolver_create_svr_boxes");
    bq_problem *p = m->p;
    bq_ctx *c = p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int k = m->k;
    const int64_t n = p->n;
    double *dy = nullptr, *deps = nullptr, *db = nullptr, *dsse = nullptr;
    long long *dnsv = nullptr, *dnheld = nullptr;
    int *count = nullptr;   // the product's column count: this call's own (the solver's nlive is 0 once every column has stopped)
    hipError_t e = hipMalloc(&dy, sizeof(double) * n);
    if (e == hipSuccess) e = hipMalloc(&deps, sizeof(double) * k);
    if (e == hipSuccess) e = hipMalloc(&db, sizeof(double) * k);
    if (e == hipSuccess) e = hipMalloc(&dsse, sizeof(double) * k);
    if (e == hipSuccess) e = hipMalloc(&dnsv, sizeof(long long) * k);
    if (e == hipSuccess) e = hipMalloc(&dnheld, sizeof(long long) * k);
    if (e == hipSuccess) e = hipMalloc(&count, sizeof(int));
    if (e == hipSuccess) e = hipMemcpyAsync(dy, y, sizeof(double) * n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(deps, epsilon, sizeof(double) * k, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(count, &k, sizeof(int), hipMemcpyHostToDevice, st);
    int rc = BQ_OK;
    if (e != hipSuccess) {
        bq_set_error("held-out scoring setup failed: %s", hipGetErrorString(e));
        rc = e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
    }
    if (rc == BQ_OK) {
        msvr_coef_kernel<<<dim3((unsigned)((n + 255) / 256), (unsigned)k), 256, 0, st>>>(m->epi, m->W, m->ldw);
        rc = bq_launch_symmw(p, false, m->W, m->ldw, k, m->slab, m->out, count);
    }
    if (rc == BQ_OK) {
        msvr_score_kernel<<<k, 1024, 0, st>>>(m->epi, m->out, m->ldw, dy, deps, db, dnsv, dsse, dnheld);
        static_assert(sizeof(long long) == sizeof(int64_t), "the counts are copied as int64_t");
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(intercept, db, sizeof(double) * k, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(sse, dsse, sizeof(double) * k, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(n_sv, dnsv, sizeof(int64_t) * k, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(n_held, dnheld, sizeof(int64_t) * k, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) {
            bq_set_error("held-out scoring: %s", hipGetErrorString(e));
            rc = BQ_ERR_HIP;
        }
    }
    if (rc == BQ_OK) rc = bq_ctx_sync(c);   // y, epsilon, k and the results are the caller's and this frame's
    else (void)bq_ctx_sync(c);
    for (void *ptr : {(void *)dy, (void *)deps, (void *)db, (void *)dsse, (void *)dnsv, (void *)dnheld, (void *)count})
        if (ptr) hipFree(ptr);
    return rc;
}

// bq_msolver_svc_heldout (data_row null: the 16-column product, msvc_heldout_kernel) and bq_msolver_pairs_heldout (the pair-routed
// product with every pair live, mpairs_heldout_kernel), after their own argument checks
static int msolver_heldout(bq_msolver *m, const unsigned char *data_row, int ncal, const int *cal_of, double *intercept,
                           int64_t *n_sv, double *A, double *B, int *iters, double *loss, int64_t *n_pos, int64_t *n_neg, int *flags,
                           double *dec) {
    BQ_ARG(ncal >= 1, "ncal must be >= 1");
    bq_problem *p = m->p;
    bq_ctx *c = p->ctx;
    const int k = m->k;
    const int64_t n = p->n;
    {   // the columns of a calibrator hold out disjoint rows: two columns may not write one entry of its sample
        std::vector<std::vector<int>> cols((size_t)ncal);
        for (int cl = 0; cl < k; ++cl) {
            BQ_ARG(cal_of[cl] >= -1 && cal_of[cl] < ncal, "cal_of entries are -1 or a calibrator in [0, ncal)");
            if (cal_of[cl] >= 0) cols[cal_of[cl]].push_back(cl);
        }
        std::vector<unsigned char> seen;
        for (const std::vector<int> &cs : cols) {
            if (cs.size() < 2) continue;
            seen.assign((size_t)n, 0);
            for (int cl : cs) {
                const unsigned char *h = m->held.data() + (size_t)cl * (size_t)n;
                for (int64_t i = 0; i < n; ++i) {
                    const unsigned char hi = h[i] && (data_row == nullptr || data_row[i]);
                    BQ_ARG(!(hi && seen[i]), "columns that share a calibrator must have disjoint held-out rows");
                    seen[i] |= hi;
                }
            }
        }
    }
    BQ_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t len = (size_t)ncal * (size_t)n;
    double *dD = nullptr, *dL = nullptr, *db = nullptr, *dA = nullptr, *dB = nullptr, *dloss = nullptr;
    long long *dnsv = nullptr, *dpos = nullptr, *dneg = nullptr;
    int *dcal = nullptr, *diters = nullptr, *dflags = nullptr;
    int *count = nullptr;   // the product's column count: this call's own (the solver's nlive is 0 once every column has stopped)
    unsigned char *drow = nullptr;
    hipError_t e = hipMalloc(&dD, sizeof(double) * len);
    if (e == hipSuccess && data_row) e = hipMalloc(&drow, (size_t)n);
    if (e == hipSuccess && data_row) e = hipMemcpyAsync(drow, data_row, (size_t)n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMalloc(&dL, sizeof(double) * len);
    if (e == hipSuccess) e = hipMalloc(&db, sizeof(double) * k);
    if (e == hipSuccess) e = hipMalloc(&dnsv, sizeof(long long) * k);
    if (e == hipSuccess) e = hipMalloc(&dcal, sizeof(int) * k);
    if (e == hipSuccess) e = hipMalloc(&dA, sizeof(double) * ncal);
    if (e == hipSuccess) e = hipMalloc(&dB, sizeof(double) * ncal);
    if (e == hipSuccess) e = hipMalloc(&dloss, sizeof(double) * ncal);
    if (e == hipSuccess) e = hipMalloc(&dpos, sizeof(long long) * ncal);
    if (e == hipSuccess) e = hipMalloc(&dneg, sizeof(long long) * ncal);
    if (e == hipSuccess) e = hipMalloc(&diters, sizeof(int) * ncal);
    if (e == hipSuccess) e = hipMalloc(&dflags, sizeof(int) * ncal);
    if (e == hipSuccess) e = hipMalloc(&count, sizeof(int));
    if (e == hipSuccess) e = hipMemsetAsync(dD, 0, sizeof(double) * len, st);
    if (e == hipSuccess) e = hipMemsetAsync(dL, 0, sizeof(double) * len, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dcal, cal_of, sizeof(int) * k, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(count, &k, sizeof(int), hipMemcpyHostToDevice, st);
    int rc = BQ_OK;
    if (e != hipSuccess) {
        bq_set_error("held-out calibration setup failed: %s", hipGetErrorString(e));
        rc = e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
    }
    if (rc == BQ_OK) {
        msvc_coef_kernel<<<dim3((unsigned)((n + 255) / 256), (unsigned)k), 256, 0, st>>>(m->epi, m->W, m->ldw);
        e = hipGetLastError();
        if (e != hipSuccess) {
            bq_set_error("held-out calibration: %s", hipGetErrorString(e));
            rc = BQ_ERR_HIP;
        }
    }
    if (rc == BQ_OK && m->plan) {
        // every pair live for this product, as bq_problem_gram_matmat_pairs has them; then the liveness of the columns' states
        // again, which is what the last iteration left (bq_launch_pairs_live is a function of the states alone)
        rc = bq_launch_pairs_all_live(m->plan, st);
        if (rc == BQ_OK) {
            rc = bq_launch_symmp(p, m->plan, false, m->W, m->ldw, m->slab, m->out);
            const int back = bq_launch_pairs_live(m->plan, m->scs, m->nlive, st);   // also when the product could not be launched
            if (rc == BQ_OK) rc = back;
        }
    } else if (rc == BQ_OK) {
        rc = bq_launch_symmw(p, false, m->W, m->ldw, k, m->slab, m->out, count);
    }
    if (rc == BQ_OK) {
        if (m->plan)
            mpairs_heldout_kernel<<<k, 1024, 0, st>>>(m->epi, m->out, m->ldw, bq_pairs_plan_pairs(m->plan),
                                                      bq_pairs_plan_tiles(m->plan), drow, dcal, dD, dL, db, dnsv);
        else
            msvc_heldout_kernel<<<k, 1024, 0, st>>>(m->epi, m->out, m->ldw, dcal, dD, dL, db, dnsv);
        e = hipGetLastError();
        if (e != hipSuccess) {
            bq_set_error("held-out calibration: %s", hipGetErrorString(e));
            rc = BQ_ERR_HIP;
        }
    }
    if (rc == BQ_OK) rc = bq_launch_platt(ncal, n, dD, dL, dA, dB, diters, dloss, dpos, dneg, dflags, st);
    if (rc == BQ_OK) {
        static_assert(sizeof(long long) == sizeof(int64_t), "the counts are copied as int64_t");
        e = hipMemcpyAsync(intercept, db, sizeof(double) * k, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(n_sv, dnsv, sizeof(int64_t) * k, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(A, dA, sizeof(double) * ncal, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(B, dB, sizeof(double) * ncal, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(loss, dloss, sizeof(double) * ncal, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(n_pos, dpos, sizeof(int64_t) * ncal, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(n_neg, dneg, sizeof(int64_t) * ncal, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(iters, diters, sizeof(int) * ncal, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(flags, dflags, sizeof(int) * ncal, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && dec) e = hipMemcpyAsync(dec, dD, sizeof(double) * len, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) {
            bq_set_error("held-out calibration: %s", hipGetErrorString(e));
            rc = BQ_ERR_HIP;
        }
    }
    if (rc == BQ_OK) rc = bq_ctx_sync(c);   // cal_of, k and the results are the caller's and this frame's
    else (void)bq_ctx_sync(c);
    for (void *ptr : {(void *)dD, (void *)dL, (void *)db, (void *)dnsv, (void *)dcal, (void *)dA, (void *)dB, (void *)dloss,
                      (void *)dpos, (void *)dneg, (void *)diters, (void *)dflags, (void *)count, (void *)drow})
        if (ptr) hipFree(ptr);
    return rc;
}

extern "C" int bq_msolver_svc_heldout(bq_msolver *m, int ncal, const int *cal_of, double *intercept, int64_t *n_sv, double *A,
                                      double *B, int *iters, double *loss, int64_t *n_pos, int64_t *n_neg, int *flags,
                                      double *dec) {
    BQ_ARG(m && cal_of && intercept && n_sv && A && B && iters && loss && n_pos && n_neg && flags, "NULL argument");
    BQ_ARG(m->svc_boxes, "held-out calibration takes a solver of bq_msolver_create_boxes");
    return msolver_heldout(m, nullptr, ncal, cal_of, intercept, n_sv, A, B, iters, loss, n_pos, n_neg, flags, dec);
}

extern "C" int bq_msolver_pairs_heldout(bq_msolver *m, const unsigned char *data_row, int ncal, const int *cal_of,
                                        double *intercept, int64_t *n_sv, double *A, double *B, int *iters, double *loss,
                                        int64_t *n_pos, int64_t *n_neg, int *flags, double *dec) {
    BQ_ARG(m && data_row && cal_of && intercept && n_sv && A && B && iters && loss && n_pos && n_neg && flags, "NULL argument");
    BQ_ARG(m->plan != nullptr && !m->held.empty(), "held-out calibration of pairs takes a solver of bq_msolver_create_pairs");
    return msolver_heldout(m, data_row, ncal, cal_of, intercept, n_sv, A, B, iters, loss, n_pos, n_neg, flags, dec);
}

static int msolver_first(bq_msolver *m) {
    bq_problem *p = m->p;
    hipStream_t st = p->ctx->stream;
    if (m->simplex) {   // x = P(0) where no start point was given, g = K x, f, the violation
        BQ_TRY(bq_sx_launch_project(m->sx_cols, m->k, m->pos, m->W, m->ldw, true, st));
        BQ_TRY(msolver_product(m, m->k));
        return bq_sx_launch_start(m->sx_cols, m->k, m->out, m->ldw, st);
    }
    const dim3 grid((unsigned)((p->n + 255) / 256), (unsigned)m->k);
    const bool svr = p->structure == BQ_SVR;
    if (svr) mstart_prep_svr_kernel<<<grid, 256, 0, st>>>(m->epi, m->W, m->ldw);
    else mstart_prep_kernel<<<grid, 256, 0, st>>>(m->epi, m->W, m->ldw);
    BQ_HIP(hipGetLastError());
    BQ_TRY(msolver_product(m, m->k));
    if (svr) mstart_finish_svr_kernel<<<grid, 256, 0, st>>>(m->epi, m->out, m->ldw);
    else mstart_finish_kernel<<<grid, 256, 0, st>>>(m->epi, m->out, m->ldw);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

static int msolver_iterate(bq_msolver *m) {
    bq_problem *p = m->p;
    hipStream_t st = p->ctx->stream;
    if (m->simplex) {
        BQ_TRY(bq_sx_launch_top(m->sx_cols, m->k, m->pos, m->nlive, st));
        BQ_TRY(bq_sx_launch_project(m->sx_cols, m->k, m->pos, m->W, m->ldw, false, st));
        BQ_TRY(msolver_product(m, m->live_host));
        return bq_sx_launch_close(m->sx_cols, m->k, m->pos, m->out, m->ldw, st);
    }
    const bq_epilogue *epi = m->epi + (m->started ? m->k : 0);
    m->started = true;
    const dim3 grid((unsigned)((p->n + 255) / 256), (unsigned)m->k);
    if (p->structure == BQ_SVR) mpgfw_update_svr_kernel<<<grid, 256, 0, st>>>(epi, m->pos, m->W, m->ldw);
    else mpgfw_update_kernel<<<grid, 256, 0, st>>>(epi, m->pos, m->W, m->ldw);
    BQ_HIP(hipGetLastError());
    BQ_TRY(msolver_product(m, m->live_host));
    mfinish_kernel<<<grid, 256, 0, st>>>(epi, m->pos, m->out, m->ldw);
    if (m->plan) return bq_launch_pairs_live(m->plan, m->scs, m->nlive, st);
    mlive_kernel<<<1, 64, 0, st>>>(m->scs, m->k, m->pos, m->nlive);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

// one iteration of every live augmented-Lagrangian column (the header comment); prep: the product's input is formed from x first
// (the first iteration of a run; every iteration of BQ_SVR)
static int msolver_al_iterate(bq_msolver *m, bool prep) {
    bq_problem *p = m->p;
    hipStream_t st = p->ctx->stream;
    const dim3 grid((unsigned)((p->n + 255) / 256), (unsigned)m->k), gridN((unsigned)((p->N + 255) / 256), (unsigned)m->k);
    if (prep || p->structure == BQ_SVR) mal_prep_kernel<<<grid, 256, 0, st>>>(m->epi, m->pos, m->W, m->ldw);
    BQ_HIP(hipGetLastError());
    BQ_TRY(msolver_product(m, m->live_host));
    mal_finish_kernel<<<grid, 256, 0, st>>>(m->epi, m->pos, m->out, m->ldw);
    mlive_kernel<<<1, 64, 0, st>>>(m->scs, m->k, m->pos, m->nlive);
    mal_update_kernel<<<gridN, 256, 0, st>>>(p->N, p->ldN, m->al_cols, m->al_prm, m->pos, m->W, m->ldw);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

// the end of a run of the augmented-Lagrangian batch: no column's stop test stays pending across the call (bq_al_flush)
static int msolver_al_flush(bq_msolver *m) {
    hipStream_t st = m->p->ctx->stream;
    mal_flush_kernel<<<dim3((unsigned)((m->p->n + 255) / 256), (unsigned)m->k), 256, 0, st>>>(m->epi);
    mlive_kernel<<<1, 64, 0, st>>>(m->scs, m->k, m->pos, m->nlive);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

extern "C" int bq_msolver_run(bq_msolver *m, int64_t max_steps, bq_iter_stat *stats, int64_t stats_cap, int64_t *n_stats,
                              int *status) {
    BQ_ARG(m && n_stats && status, "NULL argument");
    BQ_ARG(max_steps > 0, "max_steps must be > 0");
    BQ_ARG(stats == nullptr || stats_cap >= max_steps, "stats capacity must be >= max_steps");
    bq_ctx *c = m->p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    bool any = false, grown = false;
    std::vector<char> was_done(m->k);
    for (int cl = 0; cl < m->k; ++cl) {
        bq_solver *s = m->cls[cl];
        n_stats[cl] = 0;
        status[cl] = s->host.status;
        was_done[cl] = s->host.done != 0;
        any = any || !s->host.done;
        if (s->stats_cap < max_steps) {
            if (s->stats) BQ_HIP(hipFree(s->stats));
            s->stats = nullptr;
            BQ_HIP(hipMalloc(&s->stats, sizeof(bq_iter_stat) * max_steps));
            s->stats_cap = max_steps;
            grown = true;
        }
        long long hdr[2] = {s->host.iter, (long long)max_steps};
        BQ_HIP(hipMemcpyAsync(&s->sc->stat_base, hdr, sizeof(hdr), hipMemcpyHostToDevice, c->stream));
        BQ_SYNC(c);   // hdr goes out of scope
    }
    if (!any) return BQ_OK;
    if (grown) BQ_TRY(upload_epi(m));
    if (!m->initialised) {
        BQ_TRY(msolver_first(m));
        m->initialised = true;
    }
    // bq_solver_run's lagged look at the device, here at the number of live classes: about every 20 ms of estimated streaming
    const double esz = m->p->storage == BQ_F64 ? 8.0 : 4.0;
    const double passes = m->plan ? 1.0 : (double)((m->live_host + msolver_ck(m) - 1) / msolver_ck(m));
    const double iter_s = passes * (double)m->p->n * (double)m->p->n * esz * 0.5 / 5.0e12 + 30e-6 * m->k;
    int64_t poll = (int64_t)(20.0e-3 / iter_s);
    poll = poll < 1 ? 1 : (poll > 64 ? 64 : poll);
    bool pending = false;
    for (int64_t it = 0; it < max_steps; ++it) {
        BQ_TRY(m->al ? msolver_al_iterate(m, it == 0) : msolver_iterate(m));
        if ((it + 1) % poll == 0 && it + 1 < max_steps) {
            if (m->nlive_host) {
                if (pending) {
                    BQ_TRY(bq_ctx_event_sync(c, m->flag_event));
                    m->live_host = *m->nlive_host;
                    if (m->live_host == 0) break;
                }
                BQ_HIP(hipMemcpyAsync(m->nlive_host, m->nlive, sizeof(int), hipMemcpyDeviceToHost, c->stream));
                BQ_HIP(hipEventRecord(m->flag_event, c->stream));
                pending = true;
            } else {
                int nl = 0;
                BQ_HIP(hipMemcpyAsync(&nl, m->nlive, sizeof(int), hipMemcpyDeviceToHost, c->stream));
                BQ_SYNC(c);
                m->live_host = nl;
                if (nl == 0) break;
            }
        }
    }
    if (m->al) BQ_TRY(msolver_al_flush(m));
    int nl = 0;
    BQ_HIP(hipMemcpyAsync(&nl, m->nlive, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    for (int cl = 0; cl < m->k; ++cl) {
        bq_solver *s = m->cls[cl];
        BQ_HIP(hipMemcpyAsync(&s->host, s->sc, sizeof(bq_scal), hipMemcpyDeviceToHost, c->stream));
    }
    BQ_SYNC(c);
    m->live_host = nl;
    for (int cl = 0; cl < m->k; ++cl) {
        bq_solver *s = m->cls[cl];
        s->initialised = s->started = true;   // bq_solver_get / _state on the class see a solver that has run
        if (s->host.status < 0) {
            bq_set_error("non-finite values in the solver state of class %d", cl);
            return s->host.status;
        }
        const long long base = s->host.stat_base;
        int64_t rows = was_done[cl] ? 0 : s->host.iter - base + (s->host.done ? 1 : 0);   // a class done before this run has no rows
        if (rows > max_steps) rows = max_steps;
        if (rows < 0) rows = 0;
        if (stats && rows > 0) BQ_HIP(hipMemcpyAsync(stats + cl * stats_cap, s->stats, sizeof(bq_iter_stat) * rows, hipMemcpyDeviceToHost, c->stream));
        n_stats[cl] = rows;
        status[cl] = s->host.status;
    }
    BQ_SYNC(c);
    return BQ_OK;
}

extern "C" int bq_msolver_state(const bq_msolver *m, int cls, int64_t *iter, int *status, double *f_x) {
    BQ_ARG(m != nullptr && cls >= 0 && cls < m->k, "solver is NULL or class out of range");
    return bq_solver_state(m->cls[cls], iter, status, f_x);
}

extern "C" int bq_msolver_get(bq_msolver *m, int cls, int what, double *out) {
    BQ_ARG(m != nullptr && cls >= 0 && cls < m->k, "solver is NULL or class out of range");
    return bq_solver_get(m->cls[cls], what, out);
}

int bq_product_once(bq_problem *p, const char *name, int k, int64_t slots, int64_t slab_len, bool zero_out, const double *W,
                    double *out, bq_product_launch launch, void *arg) {
    bq_ctx *c = p->ctx;
    const int64_t ldw = p->ldN;
    double *dW = nullptr, *dO = nullptr, *slab = nullptr;
    int *nl = nullptr;
    hipError_t e = hipMalloc(&dW, sizeof(double) * ldw * slots);
    if (e == hipSuccess) e = hipMalloc(&dO, sizeof(double) * ldw * slots);
    if (e == hipSuccess) e = hipMalloc(&slab, sizeof(double) * slab_len);
    if (e == hipSuccess) e = hipMalloc(&nl, sizeof(int));
    if (e == hipSuccess) e = hipMemsetAsync(dW, 0, sizeof(double) * ldw * slots, c->stream);
    if (e == hipSuccess && zero_out) e = hipMemsetAsync(dO, 0, sizeof(double) * ldw * slots, c->stream);
    if (e == hipSuccess) e = hipMemcpy2DAsync(dW, sizeof(double) * ldw, W, sizeof(double) * p->n, sizeof(double) * p->n, k,
                                              hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(nl, &k, sizeof(int), hipMemcpyHostToDevice, c->stream);
    int rc = BQ_OK;
    if (e != hipSuccess) {
        bq_set_error("%s setup failed: %s", name, hipGetErrorString(e));
        rc = e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
    }
    if (rc == BQ_OK) rc = launch(arg, dW, ldw, slab, dO, nl);
    if (rc == BQ_OK) {
        e = hipMemcpy2DAsync(out, sizeof(double) * p->n, dO, sizeof(double) * ldw, sizeof(double) * p->n, k, hipMemcpyDeviceToHost,
                             c->stream);
        if (e != hipSuccess) {
            bq_set_error("%s copy: %s", name, hipGetErrorString(e));
            rc = BQ_ERR_HIP;
        }
    }
    if (rc == BQ_OK) rc = bq_ctx_sync(c);
    else (void)bq_ctx_sync(c);
    for (void *ptr : {(void *)dW, (void *)dO, (void *)slab, (void *)nl})
        if (ptr) hipFree(ptr);
    return rc;
}

static int gram_matmat(bq_problem *p, int k, const double *W, double *out, bool wide) {
    BQ_ARG(p && W && out, "NULL argument");
    BQ_ARG(k >= 1, "k must be >= 1");
    BQ_ARG(p->kernel >= 0, "not a kernel-structured problem");
    if (p->ctx->world != 1 || p->streamed || !p->symmetric) {
        bq_set_error("the multi-column product needs a single-rank context and a resident packed panel");
        return BQ_ERR_BADARG;
    }
    BQ_HIP(hipSetDevice(p->ctx->device));
    struct call { bq_problem *p; int k; bool wide; } cl{p, k, wide};
    return bq_product_once(
        p, "gram_matmat", k, bq_round_up(k, wide ? BQ_SYMMW_CK : BQ_SYMM_CK), wide ? bq_symmw_slab_len(p->nb) : bq_symm_slab_len(p->nb),
        false, W, out,
        [](void *arg, const double *dW, int64_t ldw, double *slab, double *dO, const int *nl) {
            const call *c = (const call *)arg;
            return c->wide ? bq_launch_symmw(c->p, false, dW, ldw, c->k, slab, dO, nl)
                           : bq_launch_symm(c->p, false, dW, ldw, c->k, slab, dO, nl);
        },
        &cl);
}

extern "C" int bq_problem_gram_matmat(bq_problem *p, int k, const double *W, double *out) { return gram_matmat(p, k, W, out, false); }

extern "C" int bq_problem_gram_matmat_wide(bq_problem *p, int k, const double *W, double *out) {
    return gram_matmat(p, k, W, out, true);
}

extern "C" int bq_ctx_mem_info(bq_ctx *c, int64_t *free_bytes, int64_t *total_bytes) {
    BQ_ARG(c && free_bytes && total_bytes, "NULL argument");
    BQ_HIP(hipSetDevice(c->device));
    size_t f = 0, t = 0;
    BQ_HIP(hipMemGetInfo(&f, &t));
    *free_bytes = (int64_t)f;
    *total_bytes = (int64_t)t;
    return BQ_OK;
}

extern "C" int64_t bq_problem_wide_slab_bytes(const bq_problem *p) {
    return p == nullptr ? 0 : (int64_t)sizeof(double) * bq_symmw_slab_len(p->nb);
}
