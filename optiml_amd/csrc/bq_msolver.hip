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
// update kernels owns the elements i and n + i of a target (the SVR instantiations of mstart_*_kernel, mpgfw_update_kernel), the product input is
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
// bq_msolver_create_simplex and _create_simplex2 are the batch of k capped-simplex duals on a BQ_PLAIN problem (bq_simplex.hip,
// spectral projected gradient): the nu-one-class dual, one set {0 <= x <= UB[c], sum x = mass[c]} per column (layout ONE), and the
// nu-SVC / nu-SVR duals, whose two equality rows make the set the product of two such simplices over disjoint groups of variables
// (LABELS, PAIRED).  A column's vectors x, g, d, ub are the solver's own (sx_vec: m = n entries each, 2n for PAIRED), its bq_solver
// holds the scalars and records, a bq_sx_state its step state; an iteration of all live columns is
//   top      sx_top_kernel: the record and the stop tests of every live column, then mlive_kernel's numbering — BEFORE the projection,
//            which writes the product's input to the slots of this iteration's product
//   project  sx_dir_kernel (one workgroup per column; two groups: after sx_tau_kernel, the search on one workgroup per group)
//   product  bq_launch_symmw on the signed, folded direction (n rows also for PAIRED's 2n variables, as in bq_msolver_create_svr)
//   close    sx_close_kernel
// so a run of max_steps iterations writes at most max_steps records per column, and a column's state after its last close waits
// for the next run's top.
//
// bq_msolver_create_simplex2_pairs is the two-group simplex batch on a class-sorted panel with the routed product: column c belongs
// to pair (a, b) and its groups are the row ranges of the two classes (layout BLOCKS: class b +1, class a -1, no labels vector, no
// linear term), so the nu-SVC duals of every class pair, at any number of nu, share one panel stream per iteration and a column's
// kernels walk its two classes' rows only.  pos[] stays the identity (the routed product indexes W and OUT by column): the top kernel
// takes the records and the stop tests, and the plan's live kernel follows it, before the projection.
//
// The object and what the scoring file shares with this one are in bq_msolver.h; what scores a finished batch (held-out scoring and
// calibration, the simplex offsets) is bq_mscore.hip.
#include "bq_al_update.h"
#include "bq_msolver.h"

#include <algorithm>
#include <cmath>
#include <new>

// the product input of every column from its start point, to the column's own slot
template <bool SVR>
__global__ __launch_bounds__(256) void mstart_prep_kernel(const bq_epilogue *__restrict__ epi, double *__restrict__ W, int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < e.n) W[blockIdx.y * ldw + i] = bq_mcol_input(e, i, SVR);
}

// prep_kernel + finish_kernel + grad_init_kernel of bq_pgfw_start, per class.  BQ_SVC: Qd = y o (P (y o x)) (+ diag_add x), g = Qd + q.
// BQ_SVR, both halves of panel column i: Qd = [u; -u] (+ diag_add x), g = Qd + q_c, u = P (x+ - x-)
template <bool SVR>
__global__ __launch_bounds__(256) void mstart_finish_kernel(const bq_epilogue *__restrict__ epi, const double *__restrict__ out, int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if constexpr (SVR) {
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
    } else {
        if (i >= e.N) return;
        double r = e.sgn[i] * out[blockIdx.y * ldw + i];
        if (e.diag_add != 0.0) r += e.diag_add * e.x[i];
        e.Qd[i] = r;
        e.g[i] = r + e.q[i];
    }
}

// pgfw_update_kernel (bq_vec.hip) for column blockIdx.y, writing its product input to its slot: y o d (BQ_SVC), or d+ - d- (BQ_SVR:
// the elements i and n + i of one thread, both loaded before the first use)
template <bool SVR>
__global__ __launch_bounds__(256) void mpgfw_update_kernel(const bq_epilogue *__restrict__ epi, const int *__restrict__ pos,
                                                           double *__restrict__ W, int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    if (e.sc->done) return;
    double t, tr;
    bq_epi_scalars(e, t, tr);
    const bool upd = e.do_update != 0;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= e.n) return;
    if constexpr (SVR) {
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
    } else {
        const bq_pgfw_elem a = bq_pgfw_compute(e.kind, bq_pgfw_load(e, i, upd), upd, t, tr);
        if (upd) {
            e.x[i] = a.x;
            e.g[i] = a.g;
        }
        e.d[i] = a.d;
        W[pos[blockIdx.y] * ldw + i] = e.sgn[i] * a.d;
    }
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

// ---- the augmented-Lagrangian batch
// the product input of every live column from its point: y_c o x (BQ_SVC) or x+ - x- (BQ_SVR), to the column's slot
__global__ __launch_bounds__(256) void mal_prep_kernel(const bq_epilogue *__restrict__ epi, const int *__restrict__ pos,
                                                       double *__restrict__ W, int64_t ldw) {
    const bq_epilogue &e = epi[blockIdx.y];
    if (e.sc->done) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= e.n) return;
    W[pos[blockIdx.y] * ldw + i] = bq_mcol_input(e, i, e.structure == BQ_SVR);
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

// the device tables of the columns: the records' buffers may have been re-allocated by a run with more steps
static int upload_epi(bq_msolver *m) {
    hipStream_t st = m->p->ctx->stream;
    const size_t k = (size_t)m->k;
    std::vector<bq_epilogue> h;
    std::vector<bq_al_col> cols;
    std::vector<bq_sx_col> sx;
    switch (m->method) {
        case BQ_M_SIMPLEX:
            sx.resize(k);
            for (int c = 0; c < m->k; ++c) {
                const bq_solver *s = m->cls[c];
                const int64_t n = m->p->n, mm = m->sx_m;
                const int t0 = m->sx_layout == BQ_SX_ONE ? c : 2 * c, t1 = m->sx_layout == BQ_SX_ONE ? c : 2 * c + 1;   // its groups
                double *v = m->sx_vec + 4 * mm * c;
                const long long *rg = m->sx_ranges.empty() ? nullptr : m->sx_ranges.data() + 4 * c;   // BLOCKS: off, len per group
                sx[c] = bq_sx_col{(long long)n, (long long)mm, v, v + mm, v + 2 * mm, v + 3 * mm,
                                  m->sx_sgn ? m->sx_sgn + n * c : nullptr, m->sx_q ? m->sx_q + mm * c : nullptr,
                                  {m->sx_mass[t0], m->sx_mass[t1]}, {m->sx_full[t0], m->sx_full[t1]},
                                  m->sx_has_x0 ? 1 : 0, m->sx_tau ? m->sx_tau + 8 * c : nullptr,
                                  {rg ? rg[0] : 0, rg ? rg[2] : 0}, {rg ? rg[1] : 0, rg ? rg[3] : 0}, s->sc, m->sx_state + c, s->stats};
            }
            BQ_HIP(hipMemcpyAsync(m->sx_cols, sx.data(), sizeof(bq_sx_col) * k, hipMemcpyHostToDevice, st));
            break;
        case BQ_M_AL:
            h.resize(k);
            cols.resize(k);
            for (int c = 0; c < m->k; ++c) {
                const double *sgn = m->sgn ? m->sgn + c * m->ldw : nullptr;
                h[c] = bq_al_epilogue(m->cls[c]);   // q: the column's own (V.q, bq_msolver_create_al)
                h[c].sgn = sgn;
                cols[c] = bq_al_col{m->cls[c]->al->V, m->cls[c]->sc, sgn};
            }
            BQ_HIP(hipMemcpyAsync(m->epi, h.data(), sizeof(bq_epilogue) * k, hipMemcpyHostToDevice, st));
            BQ_HIP(hipMemcpyAsync(m->al_cols, cols.data(), sizeof(bq_al_col) * k, hipMemcpyHostToDevice, st));
            break;
        case BQ_M_PGFW:
            h.resize(2 * k);
            for (int c = 0; c < m->k; ++c) {
                fill_epi(m, c, 0, h[c]);
                fill_epi(m, c, 1, h[m->k + c]);
            }
            BQ_HIP(hipMemcpyAsync(m->epi, h.data(), sizeof(bq_epilogue) * 2 * k, hipMemcpyHostToDevice, st));
            break;
    }
    BQ_SYNC(m->p->ctx);   // the host tables go out of scope
    return BQ_OK;
}

static int msolver_ck(const bq_msolver *m) { return m->product == BQ_MP_SYMM16 ? BQ_SYMMW_CK : BQ_SYMM_CK; }

static int msolver_product(bq_msolver *m, int slots) {
    bq_problem *p = m->p;
    switch (m->product) {
        case BQ_MP_PAIRS: return bq_launch_symmp(p, m->plan, p->add_one, m->W, m->ldw, m->slab, m->out);
        case BQ_MP_SYMM16: return bq_launch_symmw(p, p->add_one, m->W, m->ldw, slots, m->slab, m->out, m->nlive);
        case BQ_MP_SYMM4: break;
    }
    return bq_launch_symm(p, p->add_one, m->W, m->ldw, slots, m->slab, m->out, m->nlive);
}

static int check_labels(const double *Y, int64_t len) {
    for (int64_t i = 0; i < len; ++i) BQ_ARG(Y[i] == 1.0 || Y[i] == -1.0, "labels must be +1 or -1");
    return BQ_OK;
}

static int check_linear_terms(const double *QL, int64_t len) {
    for (int64_t i = 0; i < len; ++i) BQ_ARG(std::isfinite(QL[i]), "the linear terms must be finite");
    return BQ_OK;
}

static int msolver_check(bq_problem *p, int kind, int k, const double *Y, const double *ub, bq_msolver **out,
                         const double *QL = nullptr) {
    BQ_ARG(p && (Y || QL) && ub && out, "NULL argument");
    BQ_ARG(kind == BQ_PG || kind == BQ_FW, "the batched solver is ProjectedGradient or FrankWolfe");
    BQ_ARG(k >= 1, "k must be >= 1");
    if (QL)
        BQ_ARG(p->structure == BQ_SVR && p->kernel >= 0, "the batched SVR solver takes a kernel-built SVR problem");
    else
        BQ_ARG(p->structure == BQ_SVC && p->kernel >= 0, "the batched solver takes a kernel-built SVC problem");
    BQ_TRY(bq_need_resident_panel(p, "the batched solver", " (not streamed, not full rows)"));
    return QL ? check_linear_terms(QL, (int64_t)k * p->N) : check_labels(Y, (int64_t)k * p->n);
}

// everything of a batched solver but its columns' solvers (m->cls, m->k, m->ldw, m->method, m->product, m->plan are set): the per-column labels or
// linear terms (both null: none), the product's W / OUT / slab, the tables.  The caller destroys m on failure.
static int msolver_alloc(bq_msolver *m, const double *Y, const double *QL) {
    bq_problem *p = m->p;
    bq_ctx *c = p->ctx;
    const int k = m->k;
    const int slots = (int)bq_round_up(k, msolver_ck(m));
    // the per-column host array and its device copy: the labels (k x n -> sgn, stride ldw) or the linear terms (k x 2n -> ql, stride ldN)
    const double *col_src = QL ? QL : Y;
    double **col_dev = QL ? &m->ql : &m->sgn;
    const int64_t col_len = QL ? p->N : p->n, col_ld = QL ? p->ldN : m->ldw;
    const bool wide = m->product == BQ_MP_SYMM16;
    const int64_t slab_len = m->plan ? bq_pairs_slab_len(m->plan) : wide ? bq_symmw_slab_len(p->nb) : bq_symm_slab_len(p->nb);
    bq_owner &mem = m->mem;
    if (col_src) *col_dev = mem.dev<double>(col_ld * k);
    m->W = mem.dev<double>(m->ldw * slots);
    m->out = mem.dev<double>(m->ldw * slots);
    m->slab = mem.dev<double>(slab_len);
    m->epi = mem.dev<bq_epilogue>(2 * k);
    if (m->method == BQ_M_AL) m->al_cols = mem.dev<bq_al_col>(k);
    m->scs = mem.dev<bq_scal *>(k);
    m->pos = mem.dev<int>(k);
    m->nlive = mem.dev<int>(1);
    hipError_t e = mem.error();
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

// ub_ld: 0 (one box for every class) or the column length (class c's box at ub + c * ub_ld: m->boxes); plan: the pair-routed
// product (taken over by the solver), else the 16-column product if wide, else the 4-column one; QL: null (a BQ_SVC problem, Y: k x n
// labels), or the k x 2n linear terms of a BQ_SVR problem (Y null)
static int msolver_create(bq_problem *p, int kind, int k, const double *Y, const double *ub, int64_t ub_ld, bool wide,
                          const double *x0, double eps, int64_t max_iter, double fw_t, bq_msolver **out,
                          bq_pairs_plan *plan = nullptr, const double *QL = nullptr) {
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
    m->product = plan ? BQ_MP_PAIRS : wide ? BQ_MP_SYMM16 : BQ_MP_SYMM4;
    m->boxes = ub_ld != 0;
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

// the k x n held-out masks of *out, zeroed: no exception leaves the C ABI, and the solver does not outlive the failure
static int msolver_held_masks(bq_msolver **out) {
    bq_msolver *m = *out;
    try {
        m->held.assign((size_t)m->k * (size_t)m->p->n, 0);
    } catch (const std::bad_alloc &) {
        bq_msolver_destroy(m);
        *out = nullptr;
        bq_set_error("batched solver: no host memory for the held-out masks");
        return BQ_ERR_NOMEM;
    }
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
    BQ_TRY(msolver_held_masks(out));
    bq_msolver *m = *out;
    for (size_t i = 0; i < m->held.size(); ++i) m->held[i] = UB[i] == 0.0;
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
    BQ_TRY(msolver_held_masks(out));
    bq_msolver *s = *out;
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
    return msolver_create(p, kind, k, nullptr, UB, p->N, true, x0, eps, max_iter, fw_t, out, nullptr, QL);
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
    BQ_TRY(bq_need_resident_panel(p, "the batched solver", " (not streamed, not full rows)"));
    BQ_ARG(prm->momentum_type != BQ_MOM_NESTEROV, "Nesterov momentum is not batched: one bq_al_solver_create per column");
    BQ_ARG(a_eq == nullptr || a_ld == 0 || a_ld == p->N, "a_ld is 0 (one equality row for every column) or N (one per column)");
    if (Y) BQ_TRY(check_labels(Y, (int64_t)k * p->n));
    if (QL) BQ_TRY(check_linear_terms(QL, (int64_t)k * p->N));
    bq_ctx *c = p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    bq_msolver *m = new bq_msolver();
    m->p = p;
    p->refs += 1;
    m->method = BQ_M_AL;
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

// the problem a simplex batch takes
static int sx_check_problem(bq_problem *p) {
    BQ_ARG(p->structure == BQ_PLAIN && p->kernel >= 0, "the simplex solver takes a kernel-built BQ_PLAIN problem");
    BQ_ARG(p->diag_add == 0.0, "the simplex solver takes a problem without a diagonal term");
    return bq_need_resident_panel(p, "the batched solver", " (not streamed, not full rows)");
}
// the classes and pairs of the routed product (BLOCKS), checked by the caller
struct sx_routed {
    int ncls;
    const int *cls_tiles, *pairs;
};
// the simplex batch of any layout.  GU: the boxes of the groups (ONE: the k columns; else 2 k) as one-group columns of n rows, a row
// outside its group having none; mass: one per group; UB (k x m), sgn (LABELS: k x n, else null), q (k x m or null), x0 (k x m or
// null): the columns' vectors as the device takes them.  BLOCKS: rt, the routed product's classes and pairs (checked by the caller),
// and ranges, k x 4: the row offset and length of group 0, then of group 1
static int msolver_create_sx(bq_problem *p, int k, int layout, const double *GU, const double *UB, const double *sgn,
                             const double *mass, const double *q, const double *x0, double tol, int64_t max_iter, bq_msolver **out,
                             const sx_routed *rt = nullptr, const long long *ranges = nullptr) {
    BQ_TRY(sx_check_problem(p));
    BQ_ARG(tol >= 0.0, "tol must be >= 0");
    const bool one = layout == BQ_SX_ONE;
    const int groups = one ? k : 2 * k;
    const int64_t n = p->n, mm = layout == BQ_SX_PAIRED ? 2 * n : n;
    std::vector<int> full((size_t)groups);
    BQ_TRY(bq_sx_check(groups, n, GU, mass, full.data()));
    if (q) BQ_TRY(check_linear_terms(q, (int64_t)k * mm));
    if (x0) {   // inside its set: the box exactly, each group's mass to the rounding of a sum of n terms
        for (int64_t j = 0; j < (int64_t)k * mm; ++j) BQ_ARG(x0[j] >= 0.0 && x0[j] <= UB[j], "x0 must lie in its box");
        for (int g = 0; g < groups; ++g) {
            const double *x = x0 + (layout == BQ_SX_LABELS || layout == BQ_SX_BLOCKS ? g / 2 : g) * n;   // the n variables that hold group g
            long double sum = 0.0L;
            for (int64_t i = 0; i < n; ++i)
                if (GU[(int64_t)g * n + i] > 0.0) sum += x[i];
            BQ_ARG(std::fabs((double)sum - mass[g]) <= (double)n * 2.220446049250313e-16 * mass[g],
                   one ? "x0 must sum to its column's mass" : "x0 must sum to its group's mass");
        }
    }
    bq_ctx *c = p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    bq_msolver *m = new bq_msolver();
    m->p = p;
    p->refs += 1;
    m->kind = BQ_PG;
    m->k = k;
    m->ldw = p->ld;
    m->method = BQ_M_SIMPLEX;
    m->product = rt ? BQ_MP_PAIRS : BQ_MP_SYMM16;
    if (ranges) m->sx_ranges.assign(ranges, ranges + 4 * (size_t)k);
    m->sx_has_x0 = x0 != nullptr;
    m->sx_mass.assign(mass, mass + groups);
    m->sx_full = full;
    m->sx_m = mm;
    m->sx_layout = layout;
    const std::vector<double> zero((size_t)n, 0.0);
    int rc = rt ? bq_pairs_plan_create(p, rt->ncls, rt->cls_tiles, k, rt->pairs, &m->plan) : BQ_OK;
    for (int cl = 0; cl < k && rc == BQ_OK; ++cl) {
        bq_solver *s = nullptr;   // the column's scalars (eps = tol) and records; its vectors are sx_vec
        rc = bq_solver_create(p, BQ_PG, nullptr, zero.data(), zero.data(), tol, max_iter, 0.0, &s);
        if (rc == BQ_OK) m->cls.push_back(s);
    }
    if (rc == BQ_OK) rc = msolver_alloc(m, nullptr, nullptr);
    if (rc == BQ_OK) {
        const size_t cells = (size_t)k * (size_t)mm;
        m->sx_cols = m->mem.dev<bq_sx_col>(k);
        m->sx_state = m->mem.dev<bq_sx_state>(k);
        m->sx_rho = m->mem.dev<double>(groups);
        m->sx_counts = m->mem.dev<long long>(2 * groups);
        m->sx_vec = m->mem.dev<double>(4 * cells);
        if (!one) m->sx_tau = m->mem.dev<double>(8 * k);
        if (sgn) m->sx_sgn = m->mem.dev<double>((size_t)k * (size_t)n);
        if (q) m->sx_q = m->mem.dev<double>(cells);
        hipError_t e = m->mem.error();
        hipStream_t st = c->stream;
        if (e == hipSuccess) e = hipMemsetAsync(m->sx_state, 0, sizeof(bq_sx_state) * k, st);
        if (e == hipSuccess) e = hipMemsetAsync(m->sx_vec, 0, sizeof(double) * 4 * cells, st);
        if (e == hipSuccess && !one) e = hipMemsetAsync(m->sx_tau, 0, sizeof(double) * 8 * k, st);
        for (int cl = 0; cl < k && e == hipSuccess; ++cl) {   // x (where given) and ub of column cl
            double *v = m->sx_vec + 4 * mm * cl;
            if (x0) e = hipMemcpyAsync(v, x0 + mm * cl, sizeof(double) * mm, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(v + 3 * mm, UB + mm * cl, sizeof(double) * mm, hipMemcpyHostToDevice, st);
        }
        if (e == hipSuccess && sgn) e = hipMemcpyAsync(m->sx_sgn, sgn, sizeof(double) * k * n, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && q) e = hipMemcpyAsync(m->sx_q, q, sizeof(double) * cells, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) {
            bq_set_error("batched solver: device allocation failed: %s", hipGetErrorString(e));
            rc = BQ_ERR_NOMEM;
        }
    }
    if (rc == BQ_OK) rc = upload_epi(m);   // (its closing sync: the host arrays of the callers have been read)
    if (rc != BQ_OK) {
        bq_msolver_destroy(m);
        return rc;
    }
    *out = m;
    return BQ_OK;
}

extern "C" int bq_msolver_create_simplex(bq_problem *p, int k, const double *UB, const double *mass, const double *x0, double tol,
                                         int64_t max_iter, bq_msolver **out) {
    BQ_ARG(p && UB && mass && out, "NULL argument");
    BQ_ARG(k >= 1, "k must be >= 1");
    return msolver_create_sx(p, k, BQ_SX_ONE, UB, UB, nullptr, mass, nullptr, x0, tol, max_iter, out);
}

extern "C" int bq_msolver_create_simplex2(bq_problem *p, int k, int layout, const double *S, const double *UB, const double *mass,
                                          const double *q, const double *x0, double tol, int64_t max_iter, bq_msolver **out) {
    BQ_ARG(p && UB && mass && out, "NULL argument");
    BQ_ARG(k >= 1, "k must be >= 1");
    BQ_ARG(layout == BQ_SX_LABELS || layout == BQ_SX_PAIRED, "layout is BQ_SX_LABELS or BQ_SX_PAIRED");
    const bool paired = layout == BQ_SX_PAIRED;
    BQ_ARG(paired ? S == nullptr : S != nullptr, "the labels S belong to BQ_SX_LABELS (k x n) and to no other layout");
    const int64_t n = p->n;
    // the boxes of the 2 k groups as one-group columns of n rows: PAIRED has them so already; LABELS: a row of the other group is a
    // row without a box.  The device's labels are +1 where UB = 0 (S is not read there)
    std::vector<double> grouped, sgn;
    if (!paired) {
        grouped.assign((size_t)(2 * k) * (size_t)n, 0.0);
        sgn.assign((size_t)k * (size_t)n, 1.0);
        for (int c = 0; c < k; ++c)
            for (int64_t i = 0; i < n; ++i) {
                const double u = UB[(int64_t)c * n + i], sg = S[(int64_t)c * n + i];
                if (!(u > 0.0)) {
                    BQ_ARG(u == 0.0, "the boxes must lie in [0, 2^1021]");
                    continue;
                }
                BQ_ARG(sg == 1.0 || sg == -1.0, "S must be +1 or -1 on every row with UB > 0");
                sgn[(size_t)c * n + i] = sg;
                grouped[(size_t)(2 * c + (sg > 0.0 ? 0 : 1)) * n + i] = u;
            }
    }
    const double *GU = paired ? UB : grouped.data();
    for (int g = 0; g < 2 * k; ++g) {
        bool any = false;
        for (int64_t i = 0; i < n && !any; ++i) any = GU[(int64_t)g * n + i] > 0.0;
        BQ_ARG(any, "each of a column's two groups needs a row with UB > 0");
    }
    return msolver_create_sx(p, k, layout, GU, UB, paired ? nullptr : sgn.data(), mass, q, x0, tol, max_iter, out);
}

extern "C" int bq_msolver_create_simplex2_pairs(bq_problem *p, int ncls, const int *cls_tiles, int m, const int *pairs, const double *UB,
                                                const double *mass, const double *x0, double tol, int64_t max_iter, bq_msolver **out) {
    BQ_ARG(p && cls_tiles && pairs && UB && mass && out, "NULL argument");
    BQ_ARG(m >= 1, "m must be >= 1");
    BQ_TRY(sx_check_problem(p));
    int64_t slab_bytes = 0;
    BQ_TRY(bq_pairs_slab_bytes(p->nb, ncls, cls_tiles, m, pairs, &slab_bytes));   // validates cls_tiles and pairs
    const int64_t n = p->n;
    // the boxes of the 2 m groups as one-group columns of n rows (class b's rows, then class a's), and the groups' row ranges
    std::vector<double> grouped((size_t)(2 * m) * (size_t)n, 0.0);
    std::vector<long long> ranges(4 * (size_t)m);
    for (int c = 0; c < m; ++c) {
        long long *rg = ranges.data() + 4 * c;
        for (int t = 0; t < 2; ++t) {   // group 0: the larger class, +1
            const int cls = pairs[2 * c + (t == 0 ? 1 : 0)];
            rg[2 * t] = (long long)cls_tiles[cls] * BQ_SYM_TILE;
            rg[2 * t + 1] = std::min<long long>((long long)cls_tiles[cls + 1] * BQ_SYM_TILE, n) - rg[2 * t];
        }
        for (int64_t i = 0; i < n; ++i) {
            const double u = UB[(int64_t)c * n + i];
            const int t = (i >= rg[0] && i < rg[0] + rg[1]) ? 0 : (i >= rg[2] && i < rg[2] + rg[3]) ? 1 : -1;
            BQ_ARG(u >= 0.0 && (t >= 0 || u == 0.0), "upper bounds must be >= 0 on the pair's rows and 0 on every other row");
            if (t >= 0) grouped[(size_t)(2 * c + t) * n + i] = u;
        }
    }
    for (int g = 0; g < 2 * m; ++g) {
        bool any = false;
        for (int64_t i = 0; i < n && !any; ++i) any = grouped[(int64_t)g * n + i] > 0.0;
        BQ_ARG(any, "each of a column's two groups needs a row with UB > 0");
    }
    const sx_routed rt{ncls, cls_tiles, pairs};
    return msolver_create_sx(p, m, BQ_SX_BLOCKS, grouped.data(), UB, nullptr, mass, nullptr, x0, tol, max_iter, out, &rt, ranges.data());
}

static int msolver_first(bq_msolver *m) {
    bq_problem *p = m->p;
    hipStream_t st = p->ctx->stream;
    switch (m->method) {
        case BQ_M_SIMPLEX:   // x = P(0) per group where no start point was given, the folded x as the product's input, g, f, the violation
            BQ_TRY(bq_sx_launch_project(m->sx_cols, m->k, m->sx_layout, m->pos, m->W, m->ldw, true, st));
            BQ_TRY(msolver_product(m, m->k));
            return bq_sx_launch_start(m->sx_cols, m->k, m->sx_layout, m->out, m->ldw, st);
        case BQ_M_AL: return BQ_OK;   // no start-up product (created initialised): every iteration evaluates Q x afresh
        case BQ_M_PGFW: break;
    }
    const dim3 grid((unsigned)((p->n + 255) / 256), (unsigned)m->k);
    const bool svr = p->structure == BQ_SVR;
    if (svr) mstart_prep_kernel<true><<<grid, 256, 0, st>>>(m->epi, m->W, m->ldw);
    else mstart_prep_kernel<false><<<grid, 256, 0, st>>>(m->epi, m->W, m->ldw);
    BQ_HIP(hipGetLastError());
    BQ_TRY(msolver_product(m, m->k));
    if (svr) mstart_finish_kernel<true><<<grid, 256, 0, st>>>(m->epi, m->out, m->ldw);
    else mstart_finish_kernel<false><<<grid, 256, 0, st>>>(m->epi, m->out, m->ldw);
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


// one iteration of every live column; first_of_run: the augmented-Lagrangian batch forms its product's input from x first
static int msolver_iterate(bq_msolver *m, bool first_of_run) {
    bq_problem *p = m->p;
    hipStream_t st = p->ctx->stream;
    switch (m->method) {
        case BQ_M_SIMPLEX:
            if (m->product == BQ_MP_PAIRS) {   // pos[] stays the identity; the plan's live pairs, class slots and *nlive
                BQ_TRY(bq_sx_launch_top(m->sx_cols, m->k, nullptr, m->nlive, st));
                BQ_TRY(bq_launch_pairs_live(m->plan, m->scs, m->nlive, st));
            } else {
                BQ_TRY(bq_sx_launch_top(m->sx_cols, m->k, m->pos, m->nlive, st));
            }
            BQ_TRY(bq_sx_launch_project(m->sx_cols, m->k, m->sx_layout, m->pos, m->W, m->ldw, false, st));
            BQ_TRY(msolver_product(m, m->live_host));
            return bq_sx_launch_close(m->sx_cols, m->k, m->sx_layout, m->pos, m->out, m->ldw, st);
        case BQ_M_AL: return msolver_al_iterate(m, first_of_run);
        case BQ_M_PGFW: break;
    }
    const bq_epilogue *epi = m->epi + (m->started ? m->k : 0);
    m->started = true;
    const dim3 grid((unsigned)((p->n + 255) / 256), (unsigned)m->k);
    if (p->structure == BQ_SVR) mpgfw_update_kernel<true><<<grid, 256, 0, st>>>(epi, m->pos, m->W, m->ldw);
    else mpgfw_update_kernel<false><<<grid, 256, 0, st>>>(epi, m->pos, m->W, m->ldw);
    BQ_HIP(hipGetLastError());
    BQ_TRY(msolver_product(m, m->live_host));
    mfinish_kernel<<<grid, 256, 0, st>>>(epi, m->pos, m->out, m->ldw);
    if (m->product == BQ_MP_PAIRS) return bq_launch_pairs_live(m->plan, m->scs, m->nlive, st);
    mlive_kernel<<<1, 64, 0, st>>>(m->scs, m->k, m->pos, m->nlive);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

// the end of a run.  The augmented-Lagrangian batch: no column's stop test stays pending across the call (bq_al_flush)
static int msolver_flush(bq_msolver *m) {
    switch (m->method) {
        case BQ_M_AL: break;
        case BQ_M_PGFW:
        case BQ_M_SIMPLEX: return BQ_OK;
    }
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
            s->mem.release(s->stats);
            BQ_HIP(s->mem.dev(&s->stats, max_steps));
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
    const double passes = m->product == BQ_MP_PAIRS ? 1.0 : (double)((m->live_host + msolver_ck(m) - 1) / msolver_ck(m));
    const double iter_s = passes * (double)m->p->n * (double)m->p->n * esz * 0.5 / 5.0e12 + 30e-6 * m->k;
    int64_t poll = (int64_t)(20.0e-3 / iter_s);
    poll = poll < 1 ? 1 : (poll > 64 ? 64 : poll);
    bool pending = false;
    for (int64_t it = 0; it < max_steps; ++it) {
        BQ_TRY(msolver_iterate(m, it == 0));
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
    BQ_TRY(msolver_flush(m));
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
    if (m->method == BQ_M_SIMPLEX) {   // the column's own vectors, sx_m entries
        BQ_ARG(out, "NULL argument");
        const int v = (what == BQ_GET_X || what == BQ_GET_X_NOW) ? 0 : (what == BQ_GET_G || what == BQ_GET_G_NOW) ? 1 : what == BQ_GET_D ? 2 : -1;
        BQ_ARG(v >= 0, "vector not available for this solver");
        bq_ctx *c = m->p->ctx;
        BQ_HIP(hipSetDevice(c->device));
        BQ_HIP(hipMemcpyAsync(out, m->sx_vec + (4 * cls + v) * m->sx_m, sizeof(double) * m->sx_m, hipMemcpyDeviceToHost, c->stream));
        BQ_SYNC(c);
        return BQ_OK;
    }
    return bq_solver_get(m->cls[cls], what, out);
}
