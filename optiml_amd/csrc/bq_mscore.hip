// What scores a finished batch of the batched solver (bq_msolver.hip): from every column's point, its coefficients to the column's
// own slot (not pos[]: every column is scored, live or not), one product in which every column is live, and per column a workgroup
// of 1024 threads that sums in a fixed order (thread t the rows t, t + 1024, ... ascending, then a fixed tree: no atomics, and nothing
// of another column enters; mscore_sum).  The host side of every held-out call is one bq_score_pass (bq_score_pass.h): argument
// checks, requests, launches, finish.  bq_msolver_svr_heldout: the intercept and the held-out squared error of a column of a
// cross-validated SVR search.  bq_msolver_svc_heldout / _pairs_heldout: the intercept, the held-out decision values and their Platt
// fit (bq_platt.hip) per calibrator.  bq_msolver_simplex_offsets / _simplex2_offsets: the offsets of the nu-one-class and of the
// two-group (nu-SVC / nu-SVR) columns (bq_simplex.hip).  bq_msolver_simplex2_heldout: those offsets and the held-out accuracy
// (nu-SVC) or squared error (nu-SVR) of a column of a cross-validated nu-search.  bq_msolver_pairs_vote_heldout: the intercepts of
// the pair columns of a cross-validated one-vs-one search, their decision values on ALL rows (the 16-column product, not the routed
// one), the one-vs-one vote of every held-out row (bq_vote.h) and the held-out accuracy per (candidate, fold).
// bq_msmo_vote_heldout: the same vote and count for the pair columns of a batched SMO solver (bq_smo.hip, read through bq_msmo.h) on
// an unsorted panel: the coefficients and intercepts from the walkers' state, a row's class from its code.  bq_msmo_svr_heldout /
// bq_msmo_svc_heldout: the siblings of bq_msolver_svr_heldout / _svc_heldout for those walkers' row-list columns, the scored rows
// given as sets (held) instead of zero boxes.
#include "bq_msmo.h"
#include "bq_msolver.h"
#include "bq_score_pass.h"
#include "bq_vote.h"

#include <algorithm>
#include <cmath>
#include <vector>

static_assert(sizeof(long long) == sizeof(int64_t), "the counts are copied as int64_t");

// the coefficients of fitted_svc / fitted_svr (svm/_batched.py), their threshold and their expression
template <bool SVR>
__global__ __launch_bounds__(256) void mcoef_kernel(const bq_epilogue *__restrict__ epi, double *__restrict__ W, int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= e.n) return;
    const bool sv = SVR ? (e.x[i] > 1e-6 || e.x[e.n + i] > 1e-6) : e.x[i] > 1e-6;
    W[blockIdx.y * ldw + i] = sv ? bq_mcol_input(e, i, SVR) : 0.0;
}

// The workgroup's totals of its 1024 threads' partial sum s and count cnt, handed back to every thread in s and cnt: the two LDS
// stores, the barrier, the fixed tree (512, 256, ..., 1), the read of the totals, and the barrier after which the next pass may
// overwrite them.  Thread t's partials are of the rows t, t + 1024, ... in ascending order: no atomics, and nothing of another
// column enters
__device__ inline void mscore_sum(int tid, double &s, int &cnt) {
    __shared__ double sd[1024];
    __shared__ int sc[1024];
    sd[tid] = s;
    sc[tid] = cnt;
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if (tid < st) {
            sd[tid] += sd[tid + st];
            sc[tid] += sc[tid + st];
        }
        __syncthreads();
    }
    s = sd[0];
    cnt = sc[0];
    __syncthreads();   // every thread has read the totals: the next pass may overwrite them
}

// a row the column does not train on: ub = 0, on both halves when the column has 2n variables
template <class COL>
__device__ inline bool mscore_held(const COL &c, long long i, bool both) {
    return c.ub[i] == 0.0 && (!both || c.ub[c.n + i] == 0.0);
}

// the first pass of the held-out kernels of a column, u = K coef, t its targets (SVC: the labels e.sgn; SVR: y): over the support
// rows (x above 1e-6; SVR: on either half) S = sum (t - u) and nsv, summed by mscore_sum; returns to every thread
// b = (S - epsilon) / nsv in intercept()'s / svr_intercept()'s order (svm/_batched.py; SVC passes 0.0, and S - 0.0 has the bits of
// S), NaN for nsv = 0
template <bool SVR>
__device__ inline double mscore_intercept(const bq_epilogue &e, const double *__restrict__ u, const double *__restrict__ t,
                                          double epsilon, int tid, int &nsv) {
    const long long n = e.n;
    double s = 0.0;
    nsv = 0;
    for (long long i = tid; i < n; i += 1024) {
        const bool sv = SVR ? (e.x[i] > 1e-6 || e.x[n + i] > 1e-6) : e.x[i] > 1e-6;
        s += sv ? t[i] - u[i] : 0.0;
        nsv += sv ? 1 : 0;
    }
    mscore_sum(tid, s, nsv);
    s -= epsilon;
    return nsv > 0 ? s / (double)nsv : NAN;
}

// bq_msolver_svr_heldout, column blockIdx.x, u = out[:, column] = K coef.  Pass 1: mscore_intercept<true>.  Pass 2, the held-out
// rows (mscore_held on both halves): sse = sum (y - (u + b))^2, n_held, summed by mscore_sum.  n_sv = 0: intercept = sse = NaN.
__global__ __launch_bounds__(1024) void msvr_score_kernel(const bq_epilogue *__restrict__ epi, const double *__restrict__ out, int64_t ldw,
                                                          const double *__restrict__ y, const double *__restrict__ epsilon,
                                                          double *__restrict__ intercept, long long *__restrict__ n_sv,
                                                          double *__restrict__ sse, long long *__restrict__ n_held) {
    const bq_epilogue &e = epi[blockIdx.x];
    const double *u = out + blockIdx.x * ldw;
    const int tid = threadIdx.x;
    const long long n = e.n;
    int nsv;
    const double b = mscore_intercept<true>(e, u, y, epsilon[blockIdx.x], tid, nsv);
    double s = 0.0;
    int cnt = 0;
    for (long long i = tid; i < n; i += 1024) {
        const bool held = mscore_held(e, i, true);
        const double r = y[i] - (u[i] + b);
        s += held ? r * r : 0.0;
        cnt += held ? 1 : 0;
    }
    mscore_sum(tid, s, cnt);
    if (tid == 0) {
        intercept[blockIdx.x] = b;
        n_sv[blockIdx.x] = nsv;
        sse[blockIdx.x] = s;   // NaN with b
        n_held[blockIdx.x] = cnt;
    }
}

// bq_msolver_svc_heldout and bq_msolver_pairs_heldout, column blockIdx.x, u = out[:, column] = K coef.  Pass 1:
// mscore_intercept<false>.  Pass 2, the held-out rows: the decision value u + b and the label y to row cal_of[column] of D and L
// (row stride n; zeroed by the caller; the columns of a calibrator hold out disjoint rows, so no two workgroups write one entry).
// n_sv = 0: b = NaN.  The held-out rows are those with ub = 0 of [0, n) (pairs null), or, for column = pair (a, b) of a class-sorted
// panel, the data rows (data_row: 1; a ghost row: 0) with ub = 0 of the tile rows of a and of b — ub is 0 on every row of another
// class too, and such a row is in no pair's sample
__global__ __launch_bounds__(1024) void mheldout_kernel(const bq_epilogue *__restrict__ epi, const double *__restrict__ out,
                                                        int64_t ldw, const int *__restrict__ pairs, const int *__restrict__ ct,
                                                        const unsigned char *__restrict__ data_row, const int *__restrict__ cal_of,
                                                        double *__restrict__ D, double *__restrict__ L, double *__restrict__ intercept,
                                                        long long *__restrict__ n_sv) {
    const bq_epilogue &e = epi[blockIdx.x];
    const double *u = out + blockIdx.x * ldw;
    const int tid = threadIdx.x;
    const long long n = e.n;
    int nsv;
    const double b = mscore_intercept<false>(e, u, e.sgn, 0.0, tid, nsv);
    if (tid == 0) {
        intercept[blockIdx.x] = b;
        n_sv[blockIdx.x] = nsv;
    }
    const int cal = cal_of[blockIdx.x];
    if (cal < 0) return;
    double *d = D + (long long)cal * n, *l = L + (long long)cal * n;
    for (int side = 0; side < (pairs ? 2 : 1); ++side) {
        long long r0 = 0, r1 = n;
        if (pairs) {
            const int cls = pairs[2 * blockIdx.x + side];
            r0 = (long long)ct[cls] * BQ_SYM_TILE;
            r1 = (long long)ct[cls + 1] * BQ_SYM_TILE < n ? (long long)ct[cls + 1] * BQ_SYM_TILE : n;
        }
        for (long long i = r0 + tid; i < r1; i += 1024) {
            if ((pairs == nullptr || data_row[i]) && mscore_held(e, i, false)) {
                d[i] = u[i] + b;
                l[i] = e.sgn[i];
            }
        }
    }
}

// libsvm's calculate_rho of every group from its state on the device: r (one per group), n_sv and n_free in group order (ONE: the
// columns; else column-major k x 2)
static int msolver_sx_offsets(bq_msolver *m, double *r, int64_t *n_sv, int64_t *n_free) {
    BQ_ARG(m->initialised, "the offsets take a solver that has run");
    bq_ctx *c = m->p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int groups = m->sx_layout == BQ_SX_ONE ? m->k : 2 * m->k;
    long long *dn = m->sx_counts;
    int rc = bq_sx_launch_offsets(m->sx_cols, m->k, m->sx_layout, m->sx_rho, dn, dn + groups, st);
    if (rc == BQ_OK) {
        hipError_t e = hipMemcpyAsync(r, m->sx_rho, sizeof(double) * groups, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(n_sv, dn, sizeof(int64_t) * groups, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(n_free, dn + groups, sizeof(int64_t) * groups, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) {
            bq_set_error("simplex offsets: %s", hipGetErrorString(e));
            rc = BQ_ERR_HIP;
        }
    }
    return bq_ctx_sync_after(c, rc);
}

// the interleaved offsets (r1, r2) per column, as the device keeps them, into the caller's two arrays
static void msolver_sx_split(const std::vector<double> &r, double *r1, double *r2) {
    for (size_t cl = 0; cl < r.size() / 2; ++cl) {
        r1[cl] = r[2 * cl];
        r2[cl] = r[2 * cl + 1];
    }
}

extern "C" int bq_msolver_simplex_offsets(bq_msolver *m, double *rho, int64_t *n_sv, int64_t *n_free) {
    BQ_ARG(m && rho && n_sv && n_free, "NULL argument");
    BQ_ARG(m->method == BQ_M_SIMPLEX && m->sx_layout == BQ_SX_ONE, "the offsets take a solver of bq_msolver_create_simplex");
    return msolver_sx_offsets(m, rho, n_sv, n_free);
}

extern "C" int bq_msolver_simplex2_offsets(bq_msolver *m, double *r1, double *r2, int64_t *n_sv, int64_t *n_free) {
    BQ_ARG(m && r1 && r2 && n_sv && n_free, "NULL argument");
    BQ_ARG(m->method == BQ_M_SIMPLEX && m->sx_layout != BQ_SX_ONE, "the offsets take a solver of bq_msolver_create_simplex2");
    std::vector<double> r((size_t)(2 * m->k));
    BQ_TRY(msolver_sx_offsets(m, r.data(), n_sv, n_free));
    msolver_sx_split(r, r1, r2);
    return BQ_OK;
}

// the product's input of a two-group simplex column (bq_sx_col), to the column's own slot: the signed, folded x, S o x (LABELS: the
// device's labels are +1 where ub = 0, and x is 0 there) or x_i - x_{n + i} (PAIRED), in sx_dir_kernel's expressions.  Reads x only
template <bool PAIRED>
__global__ __launch_bounds__(256) void msx_fold_kernel(const bq_sx_col *__restrict__ cols, double *__restrict__ W, int64_t ldw) {
    const bq_sx_col &c = cols[blockIdx.y];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= c.n) return;
    W[blockIdx.y * ldw + i] = PAIRED ? c.x[i] - c.x[c.n + i] : c.sgn[i] * c.x[i];
}

// bq_msolver_simplex2_heldout, column blockIdx.x, u = out[:, column] = K b; r = the column's two offsets (r1, r2), as
// sx_offsets_kernel left them.  rho = (r1 - r2) / 2, scale = (r1 + r2) / 2.  Over the held-out rows (LABELS: ub = 0; PAIRED: ub = 0 on
// both halves): n_held, and LABELS: the rows whose prediction ((u - rho) / scale > 0: +1, else -1; a NaN or a non-positive scale as
// np.where(decision > 0, ...) takes them) equals y, sse = 0; PAIRED: sse = sum (y - (u - rho))^2, n_correct = 0.  Summed by
// mscore_sum, the matches by a second call of it beside a zero sum
template <bool PAIRED>
__global__ __launch_bounds__(1024) void msx_score_kernel(const bq_sx_col *__restrict__ cols, const double *__restrict__ out, int64_t ldw,
                                                         const double *__restrict__ y, const double *__restrict__ r,
                                                         long long *__restrict__ n_held, long long *__restrict__ n_correct,
                                                         double *__restrict__ sse) {
    const bq_sx_col &c = cols[blockIdx.x];
    const double *u = out + blockIdx.x * ldw;
    const int tid = threadIdx.x;
    const long long n = c.n;
    const double r1 = r[2 * blockIdx.x], r2 = r[2 * blockIdx.x + 1];
    const double rho = (r1 - r2) / 2, scale = (r1 + r2) / 2;
    double s = 0.0, none = 0.0;
    int held = 0, right = 0;
    for (long long i = tid; i < n; i += 1024) {
        const bool h = mscore_held(c, i, PAIRED);
        if (PAIRED) {
            const double e = y[i] - (u[i] - rho);
            s += h ? e * e : 0.0;
        } else {
            const double pred = (u[i] - rho) / scale > 0.0 ? 1.0 : -1.0;
            right += (h && pred == y[i]) ? 1 : 0;
        }
        held += h ? 1 : 0;
    }
    mscore_sum(tid, s, held);
    mscore_sum(tid, none, right);
    if (tid == 0) {
        n_held[blockIdx.x] = held;
        n_correct[blockIdx.x] = right;
        sse[blockIdx.x] = s;
    }
}

extern "C" int bq_msolver_simplex2_heldout(bq_msolver *m, const double *y, double *r1, double *r2, int64_t *n_sv, int64_t *n_free,
                                           int64_t *n_held, int64_t *n_correct, double *sse) {
    BQ_ARG(m && y && r1 && r2 && n_sv && n_free && n_held && n_correct && sse, "NULL argument");
    BQ_ARG(m->method == BQ_M_SIMPLEX && m->product == BQ_MP_SYMM16 && (m->sx_layout == BQ_SX_LABELS || m->sx_layout == BQ_SX_PAIRED),
           "held-out scoring takes a solver of bq_msolver_create_simplex2");
    BQ_ARG(m->initialised, "held-out scoring takes a solver that has run");
    bq_problem *p = m->p;
    const bool paired = m->sx_layout == BQ_SX_PAIRED;
    const int k = m->k;
    const int64_t n = p->n;
    for (int64_t i = 0; i < n; ++i) {
        if (paired) BQ_ARG(std::isfinite(y[i]), "the targets must be finite");
        else BQ_ARG(y[i] == 1.0 || y[i] == -1.0, "labels must be +1 or -1");
    }
    bq_ctx *c = p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    std::vector<double> r((size_t)(2 * k));   // (r1, r2) per column; split after the closing sync
    long long *dn = m->sx_counts;             // n_sv, then n_free, 2 k each
    bq_score_pass pass("held-out scoring", st);
    double *dy = pass.in(y, (size_t)n);
    int *count = pass.columns(k);
    pass.out_of(r.data(), m->sx_rho, (size_t)(2 * k));
    pass.out_of(n_sv, dn, (size_t)(2 * k));
    pass.out_of(n_free, dn + 2 * k, (size_t)(2 * k));
    long long *dnheld = pass.out<long long>(n_held, k), *dnright = pass.out<long long>(n_correct, k);
    double *dsse = pass.out<double>(sse, k);
    if (pass.ready() && pass.step(bq_sx_launch_offsets(m->sx_cols, k, m->sx_layout, m->sx_rho, dn, dn + 2 * k, st))) {
        // u = K b afresh: the solver's g is updated incrementally and holds the unread labels on LABELS held-out rows
        const dim3 grid((unsigned)((n + 255) / 256), (unsigned)k);
        if (paired) msx_fold_kernel<true><<<grid, 256, 0, st>>>(m->sx_cols, m->W, m->ldw);
        else msx_fold_kernel<false><<<grid, 256, 0, st>>>(m->sx_cols, m->W, m->ldw);
        if (pass.step(bq_launch_symmw(p, false, m->W, m->ldw, k, m->slab, m->out, count))) {
            if (paired) msx_score_kernel<true><<<k, 1024, 0, st>>>(m->sx_cols, m->out, m->ldw, dy, m->sx_rho, dnheld, dnright, dsse);
            else msx_score_kernel<false><<<k, 1024, 0, st>>>(m->sx_cols, m->out, m->ldw, dy, m->sx_rho, dnheld, dnright, dsse);
        }
    }
    BQ_TRY(bq_ctx_sync_after(c, pass.finish()));   // y and the results are the caller's and this frame's
    msolver_sx_split(r, r1, r2);
    return BQ_OK;
}

extern "C" int bq_msolver_svr_heldout(bq_msolver *m, const double *y, const double *epsilon, double *intercept, int64_t *n_sv,
                                      double *sse, int64_t *n_held) {
    BQ_ARG(m && y && epsilon && intercept && n_sv && sse && n_held, "NULL argument");
    BQ_ARG(bq_msolver_is_boxes(m, BQ_SVR), "held-out scoring takes a solver of bq_msolver_create_svr_boxes");
    bq_problem *p = m->p;
    bq_ctx *c = p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int k = m->k;
    const int64_t n = p->n;
    bq_score_pass pass("held-out scoring", st);
    double *dy = pass.in(y, (size_t)n), *deps = pass.in(epsilon, (size_t)k);
    double *db = pass.out<double>(intercept, k), *dsse = pass.out<double>(sse, k);
    long long *dnsv = pass.out<long long>(n_sv, k), *dnheld = pass.out<long long>(n_held, k);
    int *count = pass.columns(k);
    if (pass.ready()) {
        mcoef_kernel<true><<<dim3((unsigned)((n + 255) / 256), (unsigned)k), 256, 0, st>>>(m->epi, m->W, m->ldw);
        if (pass.step(bq_launch_symmw(p, false, m->W, m->ldw, k, m->slab, m->out, count)))
            msvr_score_kernel<<<k, 1024, 0, st>>>(m->epi, m->out, m->ldw, dy, deps, db, dnsv, dsse, dnheld);
    }
    return bq_ctx_sync_after(c, pass.finish());   // y, epsilon and the results are the caller's and this frame's
}

// bq_msolver_svc_heldout (data_row null: the 16-column product) and bq_msolver_pairs_heldout (the pair-routed product with every
// pair live), after their own argument checks
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
    bq_score_pass pass("held-out calibration", st);
    double *dD = pass.fill<double>(0, len), *dL = pass.fill<double>(0, len);
    const unsigned char *drow = data_row ? pass.in(data_row, (size_t)n) : nullptr;
    const int *dcal = pass.in(cal_of, (size_t)k);
    double *db = pass.out<double>(intercept, k);
    long long *dnsv = pass.out<long long>(n_sv, k);
    double *dA = pass.out<double>(A, ncal), *dB = pass.out<double>(B, ncal), *dloss = pass.out<double>(loss, ncal);
    long long *dpos = pass.out<long long>(n_pos, ncal), *dneg = pass.out<long long>(n_neg, ncal);
    int *diters = pass.out<int>(iters, ncal), *dflags = pass.out<int>(flags, ncal);
    pass.out_of(dec, dD, len);
    int *count = pass.columns(k);
    if (pass.ready()) {
        mcoef_kernel<false><<<dim3((unsigned)((n + 255) / 256), (unsigned)k), 256, 0, st>>>(m->epi, m->W, m->ldw);
        pass.check(hipGetLastError());
    }
    if (pass.ok() && m->plan) {
        // every pair live for this product, as bq_problem_gram_matmat_pairs has them; then the liveness of the columns' states
        // again, which is what the last iteration left (bq_launch_pairs_live is a function of the states alone)
        if (pass.step(bq_launch_pairs_all_live(m->plan, st))) {
            const int rc = bq_launch_symmp(p, m->plan, false, m->W, m->ldw, m->slab, m->out);
            const int back = bq_launch_pairs_live(m->plan, m->scs, m->nlive, st);   // also when the product could not be launched
            pass.step(rc != BQ_OK ? rc : back);
        }
    } else if (pass.ok()) {
        pass.step(bq_launch_symmw(p, false, m->W, m->ldw, k, m->slab, m->out, count));
    }
    if (pass.ok()) {
        mheldout_kernel<<<k, 1024, 0, st>>>(m->epi, m->out, m->ldw, m->plan ? bq_pairs_plan_pairs(m->plan) : nullptr,
                                            m->plan ? bq_pairs_plan_tiles(m->plan) : nullptr, drow, dcal, dD, dL, db, dnsv);
        pass.check(hipGetLastError());
    }
    if (pass.ok()) pass.step(bq_launch_platt(ncal, n, dD, dL, dA, dB, diters, dloss, dpos, dneg, dflags, st));
    return bq_ctx_sync_after(c, pass.finish());   // cal_of and the results are the caller's and this frame's
}

extern "C" int bq_msolver_svc_heldout(bq_msolver *m, int ncal, const int *cal_of, double *intercept, int64_t *n_sv, double *A,
                                      double *B, int *iters, double *loss, int64_t *n_pos, int64_t *n_neg, int *flags,
                                      double *dec) {
    BQ_ARG(m && cal_of && intercept && n_sv && A && B && iters && loss && n_pos && n_neg && flags, "NULL argument");
    BQ_ARG(bq_msolver_is_boxes(m, BQ_SVC), "held-out calibration takes a solver of bq_msolver_create_boxes");
    return msolver_heldout(m, nullptr, ncal, cal_of, intercept, n_sv, A, B, iters, loss, n_pos, n_neg, flags, dec);
}

extern "C" int bq_msolver_pairs_heldout(bq_msolver *m, const unsigned char *data_row, int ncal, const int *cal_of,
                                        double *intercept, int64_t *n_sv, double *A, double *B, int *iters, double *loss,
                                        int64_t *n_pos, int64_t *n_neg, int *flags, double *dec) {
    BQ_ARG(m && data_row && cal_of && intercept && n_sv && A && B && iters && loss && n_pos && n_neg && flags, "NULL argument");
    BQ_ARG(m->plan != nullptr && !m->held.empty(), "held-out calibration of pairs takes a solver of bq_msolver_create_pairs");
    return msolver_heldout(m, data_row, ncal, cal_of, intercept, n_sv, A, B, iters, loss, n_pos, n_neg, flags, dec);
}

// How mvote_kernel finds the class a held row must get.  mvote_tile_class, a class-sorted, tile-padded panel: a workgroup's 64 rows
// lie in one tile row, so in one class (ct: the classes' tile rows).  mvote_row_class, any panel: code[row] per lane (code: n class
// codes; read for held rows only, which lie in [0, n)).
struct mvote_tile_class {
    const int *ct;
    __device__ int operator()(int ncls, long long, bool) const {
        const int tile = (int)(((long long)blockIdx.x * BQ_VOTE_ROWS) / BQ_SYM_TILE);
        int cls = 0;
        while (cls + 1 < ncls && ct[cls + 1] <= tile) ++cls;
        return cls;
    }
};
struct mvote_row_class {
    const int *code;
    __device__ int operator()(int, long long i, bool h) const { return h ? code[i] : -1; }
};

// bq_msolver_pairs_vote_heldout and bq_msmo_vote_heldout, the rows [64 blockIdx.x, + 64) of group blockIdx.y, one thread per row.  A
// held row (held: ngroups x n) votes over the group's P columns in pair order (col_of: ngroups x P, the column of the group's pair q)
// with the decision value out[column][row] + b[column] and writes its class to pred (ngroups x n); every other row writes -1.  The
// wave counts its held rows and those whose vote is their class (class_of) into part[group][block][0 / 1].  Integer counts of
// ballots: no atomics, nothing of another group
template <class ClassOf>
__global__ __launch_bounds__(BQ_VOTE_ROWS) void mvote_kernel(int ncls, long long n, const double *__restrict__ out, int64_t ldw,
                                                             const double *__restrict__ b, const int *__restrict__ col_of,
                                                             ClassOf class_of, const unsigned char *__restrict__ held,
                                                             int *__restrict__ pred, int *__restrict__ part) {
    extern __shared__ double vote_lds[];
    const int g = blockIdx.y, tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * BQ_VOTE_ROWS + tid;
    const int *cols = col_of + (long long)g * (ncls * (ncls - 1) / 2);
    const bool h = i < n && held[(long long)g * n + i] != 0;
    int p = -1;
    if (h) {
        const double *u = out + i;
        p = bq_ovo_vote_row(ncls, [=](int k) { return u[cols[k] * ldw] + b[cols[k]]; }, vote_lds, tid, nullptr);
    }
    if (i < n) pred[(long long)g * n + i] = p;
    const int cls = class_of(ncls, i, h);
    const unsigned long long hm = __ballot(h), rm = __ballot(h && p == cls);
    if (tid == 0) {
        int *dst = part + 2 * ((long long)g * gridDim.x + blockIdx.x);
        dst[0] = __popcll(hm);
        dst[1] = __popcll(rm);
    }
}

// group blockIdx.x: the sums of mvote_kernel's nblk pairs of counts (thread t the blocks t, t + 1024, ... ascending, then a fixed
// tree of integers) -> n_held, n_correct; a NaN among the intercepts of the group's P columns -> n_correct = -1
__global__ __launch_bounds__(1024) void mvote_count_kernel(int P, int nblk, const int *__restrict__ part, const double *__restrict__ b,
                                                           const int *__restrict__ col_of, long long *__restrict__ n_held,
                                                           long long *__restrict__ n_correct) {
    __shared__ int sh[1024], sr[1024], sb[1024];
    const int g = blockIdx.x, tid = threadIdx.x;
    int h = 0, r = 0, bad = 0;
    for (int j = tid; j < nblk; j += 1024) {
        h += part[2 * ((long long)g * nblk + j)];
        r += part[2 * ((long long)g * nblk + j) + 1];
    }
    for (int q = tid; q < P; q += 1024) bad |= std::isnan(b[col_of[(long long)g * P + q]]) ? 1 : 0;
    sh[tid] = h;
    sr[tid] = r;
    sb[tid] = bad;
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if (tid < st) {
            sh[tid] += sh[tid + st];
            sr[tid] += sr[tid + st];
            sb[tid] |= sb[tid + st];
        }
        __syncthreads();
    }
    if (tid == 0) {
        n_held[g] = sh[0];
        n_correct[g] = sb[0] ? -1 : sr[0];
    }
}

extern "C" int bq_msolver_pairs_vote_heldout(bq_msolver *m, const unsigned char *data_row, int ngroups, const int *group_of,
                                             const unsigned char *held, double *intercept, int64_t *n_sv, int64_t *n_held,
                                             int64_t *n_correct, int *pred) {
    BQ_ARG(m && data_row && group_of && held && intercept && n_sv && n_held && n_correct, "NULL argument");
    BQ_ARG(m->method == BQ_M_PGFW && m->plan != nullptr && !m->held.empty(),
           "the held-out vote takes a solver of bq_msolver_create_pairs");
    bq_problem *p = m->p;
    bq_ctx *c = p->ctx;
    const int k = m->k, ncls = bq_pairs_plan_ncls(m->plan);
    const int64_t n = p->n;
    const int P = ncls * (ncls - 1) / 2;
    BQ_ARG(ncls <= BQ_VOTE_MAX_CLS, "the one-vs-one vote takes at most 64 classes");
    BQ_ARG(ngroups >= 1 && ngroups <= 65535 && (int64_t)ngroups * P == k, "the columns must be ngroups x the ncls (ncls - 1) / 2 pairs");
    const int *hp = bq_pairs_plan_host_pairs(m->plan), *hct = bq_pairs_plan_host_tiles(m->plan);
    std::vector<int> col_of((size_t)k, -1);   // ngroups x P: the column of (group, pair number in ovo_pairs order)
    for (int cl = 0; cl < k; ++cl) {
        BQ_ARG(group_of[cl] >= 0 && group_of[cl] < ngroups, "group_of entries are groups in [0, ngroups)");
        const int a = hp[2 * cl], b = hp[2 * cl + 1];
        int &slot = col_of[(size_t)group_of[cl] * P + (a * ncls - a * (a + 1) / 2 + (b - a - 1))];
        BQ_ARG(slot < 0, "a group must hold every pair exactly once");
        slot = cl;
    }   // (k = ngroups x P columns in k distinct slots: every slot is filled)
    // a held row is a data row that no column of its group trained on: UB = 0 there.  A column's box is 0 outside its pair's classes
    // (checked at creation), and m->held has it on the rows of the pair's classes
    for (int g = 0; g < ngroups; ++g) {
        const unsigned char *hg = held + (size_t)g * (size_t)n;
        for (int cls = 0; cls < ncls; ++cls) {
            const int64_t r0 = (int64_t)hct[cls] * BQ_SYM_TILE, r1 = std::min<int64_t>((int64_t)hct[cls + 1] * BQ_SYM_TILE, n);
            bool any = false;
            for (int64_t i = r0; i < r1; ++i) {
                BQ_ARG(!hg[i] || data_row[i], "a held row must be a data row");
                any |= hg[i] != 0;
            }
            if (!any) continue;
            for (int q = 0; q < P; ++q) {
                const int cl = col_of[(size_t)g * P + q];
                if (hp[2 * cl] != cls && hp[2 * cl + 1] != cls) continue;
                const unsigned char *zero = m->held.data() + (size_t)cl * (size_t)n;
                for (int64_t i = r0; i < r1; ++i) BQ_ARG(!hg[i] || zero[i], "a held row must have UB = 0 in every column of its group");
            }
        }
    }
    BQ_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // The product's own scratch: symmw_tiles_kernel stages all 16 slots of a chunk whatever is live, and a pair solver's W / out have
    // round_up(k, 4) slots and its slab the routed product's layout
    const int64_t slots = bq_round_up(k, BQ_SYMMW_CK), ldw = m->ldw;
    const int nblk = (int)((n + BQ_VOTE_ROWS - 1) / BQ_VOTE_ROWS);
    bq_score_pass pass("held-out vote", st);
    double *W = pass.fill<double>(0, ldw * slots), *OUT = pass.fill<double>(0, ldw * slots);
    double *slab = pass.dev<double>(bq_symmw_slab_len(p->nb));
    double *db = pass.out<double>(intercept, k);
    long long *dnsv = pass.out<long long>(n_sv, k);
    long long *dnheld = pass.out<long long>(n_held, ngroups), *dnright = pass.out<long long>(n_correct, ngroups);
    int *dpred = pass.out<int>(pred, (size_t)ngroups * (size_t)n);   // (pred may be null: the rows' classes stay on the device)
    const int *dcal = pass.fill<int>(0xff, k);                       // -1: mheldout_kernel stops after the intercept
    const int *dcol = pass.in(col_of.data(), (size_t)k);
    int *part = pass.dev<int>((size_t)2 * ngroups * nblk);
    const unsigned char *dheld = pass.in(held, (size_t)ngroups * (size_t)n);
    int *count = pass.columns(k);
    if (pass.ready()) {
        mcoef_kernel<false><<<dim3((unsigned)((n + 255) / 256), (unsigned)k), 256, 0, st>>>(m->epi, W, ldw);
        // u on ALL rows: the routed product leaves 0 outside a pair's classes
        if (pass.step(bq_launch_symmw(p, false, W, ldw, k, slab, OUT, count))) {
            mheldout_kernel<<<k, 1024, 0, st>>>(m->epi, OUT, ldw, nullptr, nullptr, nullptr, dcal, nullptr, nullptr, db, dnsv);
            mvote_kernel<<<dim3((unsigned)nblk, (unsigned)ngroups), BQ_VOTE_ROWS, bq_vote_lds_bytes(ncls), st>>>(
                ncls, (long long)n, OUT, ldw, db, dcol, mvote_tile_class{bq_pairs_plan_tiles(m->plan)}, dheld, dpred, part);
            mvote_count_kernel<<<ngroups, 1024, 0, st>>>(P, nblk, part, db, dcol, dnheld, dnright);
        }
    }
    return bq_ctx_sync_after(c, pass.finish());   // held, the tables and the results are the caller's and this frame's
}

// bq_msmo_vote_heldout / _svr_heldout / _svc_heldout, column blockIdx.x of a batched SMO solver, from the state its walker left (Y,
// A: k x n; AM: k x n, SVR only; sc: k).  The coefficients of fitted_smo_svc (svm/_batched.py: a y where a > 1e-6, else 0) or, SVR, of
// _svr_attributes (a+ - a- where a+ > 1e-6 or a- > 1e-6, else 0) to the column's slot of W (stride ldw; its tail stays 0), n_sv their
// count (thread t the rows t, t + 1024, ... ascending, then a fixed tree of integers), and from the column's record the intercept
// -(b_low + b_up) / 2 (SVR: +(b_low + b_up) / 2), bq_msmo_get's BQ_SMO_SCALARS[5] statement.  flag: the intercept, or NaN for a
// column whose walker failed (err_flag) — what mvote_count_kernel and the two score kernels read as a failed fit.  intercept may
// be null: the two held-out scorers report flag
template <bool SVR>
__global__ __launch_bounds__(1024) void msmo_coef_kernel(long long n, const double *__restrict__ Y, const double *__restrict__ A,
                                                         const double *__restrict__ AM, const bq_smo_scal *__restrict__ sc,
                                                         double *__restrict__ W, int64_t ldw, double *__restrict__ intercept,
                                                         double *__restrict__ flag, long long *__restrict__ n_sv) {
    __shared__ int cnt[1024];
    const int tid = threadIdx.x;
    const long long c = blockIdx.x;
    const double *y = Y + c * n, *a = A + c * n, *am = SVR ? AM + c * n : nullptr;
    double *w = W + c * ldw;
    int mine = 0;
    for (long long i = tid; i < n; i += 1024) {
        bool sv;
        double coef;
        if (SVR) {
            sv = a[i] > 1e-6 || am[i] > 1e-6;
            coef = a[i] - am[i];
        } else {
            sv = a[i] > 1e-6;
            coef = a[i] * y[i];
        }
        w[i] = sv ? coef : 0.0;
        mine += sv ? 1 : 0;
    }
    cnt[tid] = mine;
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if (tid < st) cnt[tid] += cnt[tid + st];
        __syncthreads();
    }
    if (tid == 0) {
        const double b = SVR ? (sc[c].b_low + sc[c].b_up) / 2 : -(sc[c].b_low + sc[c].b_up) / 2;
        if (intercept) intercept[c] = b;
        flag[c] = sc[c].err_flag ? NAN : b;
        n_sv[c] = cnt[0];
    }
}

// bq_msmo_svr_heldout, column blockIdx.x, u = out[:, column] = K coef, y the column's targets (the solver's Y), b = flag[column]
// (NaN: the walker failed).  Over the rows of set set_of[column] (held: nsets x n bytes; -1: no row): sse = sum (y - (u + b))^2 and
// n_held, summed by mscore_sum.  A failed column: sse = NaN, also when it scores no row
__global__ __launch_bounds__(1024) void msmo_svr_score_kernel(long long n, const double *__restrict__ Y, const double *__restrict__ out,
                                                              int64_t ldw, const double *__restrict__ flag,
                                                              const int *__restrict__ set_of, const unsigned char *__restrict__ held,
                                                              double *__restrict__ sse, long long *__restrict__ n_held) {
    const int tid = threadIdx.x;
    const long long c = blockIdx.x;
    const double *y = Y + c * n, *u = out + c * ldw;
    const double b = flag[c];
    const int set = set_of[c];
    double s = 0.0;
    int cnt = 0;
    if (set >= 0) {
        const unsigned char *h = held + (long long)set * n;
        for (long long i = tid; i < n; i += 1024) {
            const bool hi = h[i] != 0;
            const double r = y[i] - (u[i] + b);
            s += hi ? r * r : 0.0;
            cnt += hi ? 1 : 0;
        }
    }
    mscore_sum(tid, s, cnt);
    if (tid == 0) {
        sse[c] = std::isnan(b) ? NAN : s;
        n_held[c] = cnt;
    }
}

// bq_msmo_svc_heldout, column blockIdx.x, u = out[:, column] = K coef, y the column's labels (the solver's Y), b = flag[column]
// (NaN: the walker failed, and so are its decision values).  On the rows of set set_of[column] the decision value u + b and the
// label y to row cal_of[column] of D and L (row stride n; zeroed by the caller; the columns of a calibrator score disjoint rows, so
// no two workgroups write one entry).  set_of or cal_of -1: nothing is written
__global__ __launch_bounds__(1024) void msmo_svc_score_kernel(long long n, const double *__restrict__ Y, const double *__restrict__ out,
                                                              int64_t ldw, const double *__restrict__ flag,
                                                              const int *__restrict__ set_of, const unsigned char *__restrict__ held,
                                                              const int *__restrict__ cal_of, double *__restrict__ D,
                                                              double *__restrict__ L) {
    const int tid = threadIdx.x;
    const long long c = blockIdx.x;
    const int set = set_of[c], cal = cal_of[c];
    if (set < 0 || cal < 0) return;
    const double *y = Y + c * n, *u = out + c * ldw;
    const unsigned char *h = held + (long long)set * n;
    const double b = flag[c];
    double *d = D + (long long)cal * n, *l = L + (long long)cal * n;
    for (long long i = tid; i < n; i += 1024) {
        if (h[i]) {
            d[i] = u[i] + b;
            l[i] = y[i];
        }
    }
}

// The argument checks bq_msmo_svr_heldout and bq_msmo_svc_heldout share, on the host against the solver's host copies of its lists:
// the task, nsets, the entries of set_of, the resident panel, and per scoring column a row list that holds none of its scored rows
static int msmo_heldout_args(const bq_msmo_view &v, int task, const char *what, int nsets, const int *set_of,
                             const unsigned char *held) {
    BQ_ARG(v.task == task, task == BQ_SVR ? "held-out scoring takes a BQ_SVR solver" : "held-out calibration takes a BQ_SVC solver");
    BQ_ARG(nsets >= 1, "nsets must be >= 1");
    for (int cl = 0; cl < v.k; ++cl) BQ_ARG(set_of[cl] >= -1 && set_of[cl] < nsets, "set_of entries are -1 or a set in [0, nsets)");
    BQ_TRY(bq_need_resident_panel(v.p, what));
    for (int cl = 0; cl < v.k; ++cl) {
        if (set_of[cl] < 0) continue;
        BQ_ARG(v.row_ptr != nullptr, "a column that scores rows needs a row list: without one it trains on every row");
        const unsigned char *h = held + (size_t)set_of[cl] * (size_t)v.n;
        for (int64_t q = v.row_ptr[cl]; q < v.row_ptr[cl + 1]; ++q)
            BQ_ARG(!h[v.rows[q]], "a scored row must not be in the column's own row list");
    }
    return BQ_OK;
}

extern "C" int bq_msmo_svr_heldout(bq_msmo *s, int nsets, const int *set_of, const unsigned char *held, double *intercept,
                                   int64_t *n_sv, double *sse, int64_t *n_held) {
    BQ_ARG(s && set_of && held && intercept && n_sv && sse && n_held, "NULL argument");
    const bq_msmo_view v = bq_msmo_view_of(s);
    BQ_TRY(msmo_heldout_args(v, BQ_SVR, "held-out scoring", nsets, set_of, held));
    bq_problem *p = v.p;
    bq_ctx *c = p->ctx;
    const int k = v.k;
    const int64_t n = v.n;
    BQ_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // the product's own scratch: every column in its own slot of a chunk of 16, the padding slots zero
    const int64_t slots = bq_round_up(k, BQ_SYMMW_CK), ldw = p->ldN;
    bq_score_pass pass("held-out scoring", st);
    double *W = pass.fill<double>(0, ldw * slots), *OUT = pass.fill<double>(0, ldw * slots);
    double *slab = pass.dev<double>(bq_symmw_slab_len(p->nb));
    double *dflag = pass.out<double>(intercept, k);   // NaN for a failed walker
    double *dsse = pass.out<double>(sse, k);
    long long *dnsv = pass.out<long long>(n_sv, k), *dnheld = pass.out<long long>(n_held, k);
    const int *dset = pass.in(set_of, (size_t)k);
    const unsigned char *dheld = pass.in(held, (size_t)nsets * (size_t)n);
    int *count = pass.columns(k);
    if (pass.ready()) {
        msmo_coef_kernel<true><<<k, 1024, 0, st>>>((long long)n, v.Y, v.A, v.AM, v.sc, W, ldw, nullptr, dflag, dnsv);
        if (pass.step(bq_launch_symmw(p, false, W, ldw, k, slab, OUT, count)))
            msmo_svr_score_kernel<<<k, 1024, 0, st>>>((long long)n, v.Y, OUT, ldw, dflag, dset, dheld, dsse, dnheld);
    }
    return bq_ctx_sync_after(c, pass.finish());   // the tables and the results are the caller's and this frame's
}

extern "C" int bq_msmo_svc_heldout(bq_msmo *s, int nsets, const int *set_of, const unsigned char *held, int ncal, const int *cal_of,
                                   double *intercept, int64_t *n_sv, double *A, double *B, int *iters, double *loss, int64_t *n_pos,
                                   int64_t *n_neg, int *flags, double *dec) {
    BQ_ARG(s && set_of && held && cal_of && intercept && n_sv && A && B && iters && loss && n_pos && n_neg && flags, "NULL argument");
    const bq_msmo_view v = bq_msmo_view_of(s);
    BQ_TRY(msmo_heldout_args(v, BQ_SVC, "held-out calibration", nsets, set_of, held));
    BQ_ARG(ncal >= 1, "ncal must be >= 1");
    bq_problem *p = v.p;
    bq_ctx *c = p->ctx;
    const int k = v.k;
    const int64_t n = v.n;
    {   // the columns of a calibrator score disjoint rows: two columns may not write one entry of its sample
        std::vector<std::vector<int>> cols((size_t)ncal);
        for (int cl = 0; cl < k; ++cl) {
            BQ_ARG(cal_of[cl] >= -1 && cal_of[cl] < ncal, "cal_of entries are -1 or a calibrator in [0, ncal)");
            if (cal_of[cl] >= 0 && set_of[cl] >= 0) cols[cal_of[cl]].push_back(cl);
        }
        std::vector<unsigned char> seen;
        for (const std::vector<int> &cs : cols) {
            if (cs.size() < 2) continue;
            seen.assign((size_t)n, 0);
            for (int cl : cs) {
                const unsigned char *h = held + (size_t)set_of[cl] * (size_t)n;
                for (int64_t i = 0; i < n; ++i) {
                    BQ_ARG(!(h[i] && seen[i]), "columns that share a calibrator must score disjoint rows");
                    seen[i] |= h[i];
                }
            }
        }
    }
    BQ_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int64_t slots = bq_round_up(k, BQ_SYMMW_CK), ldw = p->ldN;
    const size_t len = (size_t)ncal * (size_t)n;
    std::vector<int> tables((size_t)2 * k);   // set_of, then cal_of
    std::copy(set_of, set_of + k, tables.begin());
    std::copy(cal_of, cal_of + k, tables.begin() + k);
    // bq_scratch hands out 16 buffers a call: the product's input and output share one, the calibrators' two samples another,
    // the two tables a third
    bq_score_pass pass("held-out calibration", st);
    double *W = pass.fill<double>(0, 2 * ldw * slots), *OUT = W ? W + ldw * slots : nullptr;
    double *slab = pass.dev<double>(bq_symmw_slab_len(p->nb));
    double *dD = pass.fill<double>(0, 2 * len), *dL = dD ? dD + len : nullptr;
    double *dflag = pass.out<double>(intercept, k);   // NaN for a failed walker
    long long *dnsv = pass.out<long long>(n_sv, k);
    double *dA = pass.out<double>(A, ncal), *dB = pass.out<double>(B, ncal), *dloss = pass.out<double>(loss, ncal);
    long long *dpos = pass.out<long long>(n_pos, ncal), *dneg = pass.out<long long>(n_neg, ncal);
    int *diters = pass.out<int>(iters, ncal), *dflags = pass.out<int>(flags, ncal);
    pass.out_of(dec, dD, len);
    const int *dset = pass.in(tables.data(), tables.size()), *dcal = dset ? dset + k : nullptr;
    const unsigned char *dheld = pass.in(held, (size_t)nsets * (size_t)n);
    int *count = pass.columns(k);
    if (pass.ready()) {
        msmo_coef_kernel<false><<<k, 1024, 0, st>>>((long long)n, v.Y, v.A, nullptr, v.sc, W, ldw, nullptr, dflag, dnsv);
        if (pass.step(bq_launch_symmw(p, false, W, ldw, k, slab, OUT, count))) {
            msmo_svc_score_kernel<<<k, 1024, 0, st>>>((long long)n, v.Y, OUT, ldw, dflag, dset, dheld, dcal, dD, dL);
            pass.check(hipGetLastError());
            if (pass.ok()) pass.step(bq_launch_platt(ncal, n, dD, dL, dA, dB, diters, dloss, dpos, dneg, dflags, st));
        }
    }
    return bq_ctx_sync_after(c, pass.finish());   // the tables and the results are the caller's and this frame's
}

extern "C" int bq_msmo_vote_heldout(bq_msmo *s, int ncls, const int *code, int ngroups, const int *group_of, const int *pair_of,
                                    const unsigned char *held, double *intercept, int64_t *n_sv, int64_t *n_held,
                                    int64_t *n_correct, int *pred) {
    BQ_ARG(s && code && group_of && pair_of && held && intercept && n_sv && n_held && n_correct, "NULL argument");
    const bq_msmo_view v = bq_msmo_view_of(s);
    BQ_ARG(v.task == BQ_SVC, "the held-out vote takes a BQ_SVC solver");
    BQ_ARG(ncls >= 2 && ncls <= BQ_VOTE_MAX_CLS, "the one-vs-one vote takes 2 to 64 classes");
    bq_problem *p = v.p;
    bq_ctx *c = p->ctx;
    const int k = v.k;
    const int64_t n = v.n;
    const int P = ncls * (ncls - 1) / 2;
    BQ_ARG(ngroups >= 1 && ngroups <= 65535 && (int64_t)ngroups * P == k, "the columns must be ngroups x the ncls (ncls - 1) / 2 pairs");
    BQ_TRY(bq_need_resident_panel(p, "the held-out vote"));
    BQ_ARG(v.row_ptr != nullptr && v.sign != nullptr, "every column needs a row list");
    std::vector<int> pairs((size_t)2 * P);   // ovo_pairs order
    for (int a = 0, q = 0; a < ncls; ++a)
        for (int b = a + 1; b < ncls; ++b, ++q) {
            pairs[2 * q] = a;
            pairs[2 * q + 1] = b;
        }
    std::vector<int> col_of((size_t)k, -1);   // ngroups x P: the column of (group, pair number)
    for (int cl = 0; cl < k; ++cl) {
        BQ_ARG(group_of[cl] >= 0 && group_of[cl] < ngroups, "group_of entries are groups in [0, ngroups)");
        BQ_ARG(pair_of[cl] >= 0 && pair_of[cl] < P, "pair_of entries are pair numbers in [0, ncls (ncls - 1) / 2)");
        int &slot = col_of[(size_t)group_of[cl] * P + pair_of[cl]];
        BQ_ARG(slot < 0, "a group must hold every pair exactly once");
        slot = cl;
    }   // (k = ngroups x P columns in k distinct slots: every slot is filled)
    for (int64_t i = 0; i < n; ++i) BQ_ARG(code[i] >= 0 && code[i] < ncls, "code entries are classes in [0, ncls)");
    for (int cl = 0; cl < k; ++cl) {
        const int a = pairs[2 * pair_of[cl]], b = pairs[2 * pair_of[cl] + 1];
        for (int64_t q = v.row_ptr[cl]; q < v.row_ptr[cl + 1]; ++q) {
            const int cd = code[v.rows[q]];
            BQ_ARG(cd == a || cd == b, "a column's row list holds a row of a class outside its pair");
            BQ_ARG(v.sign[q] == (cd == b ? 1 : -1), "a column's labels must be +1 on its pair's larger class and -1 on the smaller");
        }
    }
    {
        std::vector<unsigned char> trained((size_t)n);
        for (int g = 0; g < ngroups; ++g) {
            std::fill(trained.begin(), trained.end(), (unsigned char)0);
            for (int q = 0; q < P; ++q) {
                const int cl = col_of[(size_t)g * P + q];
                for (int64_t r = v.row_ptr[cl]; r < v.row_ptr[cl + 1]; ++r) trained[(size_t)v.rows[r]] = 1;
            }
            const unsigned char *hg = held + (size_t)g * (size_t)n;
            for (int64_t i = 0; i < n; ++i) BQ_ARG(!(hg[i] && trained[(size_t)i]), "a held row must not be in a row list of its group");
        }
    }
    BQ_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // the product's own scratch: every column in its own slot of a chunk of 16, the padding slots zero
    const int64_t slots = bq_round_up(k, BQ_SYMMW_CK), ldw = p->ldN;
    const int nblk = (int)((n + BQ_VOTE_ROWS - 1) / BQ_VOTE_ROWS);
    bq_score_pass pass("held-out vote", st);
    double *W = pass.fill<double>(0, ldw * slots), *OUT = pass.fill<double>(0, ldw * slots);
    double *slab = pass.dev<double>(bq_symmw_slab_len(p->nb));
    double *db = pass.out<double>(intercept, k);
    double *dflag = pass.dev<double>(k);
    long long *dnsv = pass.out<long long>(n_sv, k);
    long long *dnheld = pass.out<long long>(n_held, ngroups), *dnright = pass.out<long long>(n_correct, ngroups);
    int *dpred = pass.out<int>(pred, (size_t)ngroups * (size_t)n);   // (pred may be null: the rows' classes stay on the device)
    const int *dcol = pass.in(col_of.data(), (size_t)k);
    const int *dcode = pass.in(code, (size_t)n);
    int *part = pass.dev<int>((size_t)2 * ngroups * nblk);
    const unsigned char *dheld = pass.in(held, (size_t)ngroups * (size_t)n);
    int *count = pass.columns(k);
    if (pass.ready()) {
        msmo_coef_kernel<false><<<k, 1024, 0, st>>>((long long)n, v.Y, v.A, nullptr, v.sc, W, ldw, db, dflag, dnsv);
        if (pass.step(bq_launch_symmw(p, false, W, ldw, k, slab, OUT, count))) {
            mvote_kernel<<<dim3((unsigned)nblk, (unsigned)ngroups), BQ_VOTE_ROWS, bq_vote_lds_bytes(ncls), st>>>(
                ncls, (long long)n, OUT, ldw, db, dcol, mvote_row_class{dcode}, dheld, dpred, part);
            mvote_count_kernel<<<ngroups, 1024, 0, st>>>(P, nblk, part, dflag, dcol, dnheld, dnright);
        }
    }
    return bq_ctx_sync_after(c, pass.finish());   // the tables and the results are the caller's and this frame's
}
