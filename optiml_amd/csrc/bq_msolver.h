// The batched solver's object (bq_msolver.hip: creation and iteration; bq_mscore.hip: what scores a finished batch).
#pragma once
#include "bq_al.h"
#include "bq_common.h"
#include "bq_epilogue.h"
#include "bq_simplex.h"

#include <vector>

// what mal_update_kernel takes of an augmented-Lagrangian column (al_update_kernel's arguments)
struct bq_al_col {
    bq_al_vecs V;
    bq_scal *sc;
    const double *sgn;   // the column's labels (BQ_SVC), else null
};

// A flavour is a method, a product and `boxes`; the creation functions make exactly these:
//   _create, _create_svr            PGFW     SYMM4
//   _create_boxes, _svr_boxes       PGFW     SYMM16   boxes
//   _create_pairs                   PGFW     PAIRS    boxes
//   _create_al                      AL       SYMM4
//   _create_simplex, _simplex2      SIMPLEX  SYMM16   sx_layout: ONE; LABELS or PAIRED
//   _create_simplex2_pairs          SIMPLEX  PAIRS    sx_layout: BLOCKS
enum bq_mmethod {
    BQ_M_PGFW,      // ProjectedGradient / FrankWolfe columns (bq_msolver::kind says which)
    BQ_M_AL,        // augmented-Lagrangian columns (bq_al.hip); epi: k entries of kind 2
    BQ_M_SIMPLEX,   // capped-simplex columns of one or two groups (bq_simplex.hip: bq_sx_col), which own their vectors (sx_vec)
};
enum bq_mproduct {
    BQ_MP_SYMM4,    // bq_symm.hip, 4 columns per panel stream
    BQ_MP_SYMM16,   // bq_symmw.hip, 16 columns per panel stream
    BQ_MP_PAIRS,    // bq_symmp.hip, the pair-routed product of `plan`
};

struct bq_msolver {
    bq_problem *p = nullptr;
    bq_owner mem;   // the device buffers below (the columns' solvers in `cls` and the plan own theirs)
    int kind = BQ_PG, k = 0;
    bq_mmethod method = BQ_M_PGFW;
    bq_mproduct product = BQ_MP_SYMM4;
    bool boxes = false;   // one box per column (UB: k x n or k x 2n, lb = 0); a column's held-out rows have ub = 0
    // bq_msolver_create_boxes: k x n, 1 where UB is 0 (the column's held-out rows), as given at creation; bq_msolver_create_pairs: the
    // same on the rows of the pair's classes and 0 on every other row (bq_msolver_pairs_heldout)
    std::vector<unsigned char> held;
    bq_pairs_plan *plan = nullptr;   // BQ_MP_PAIRS: the plan of the routed product (the solver's to destroy)
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
    bq_al_params al_prm = {};
    bq_al_col *al_cols = nullptr;       // BQ_M_AL, k: what mal_update_kernel reads of a column
    // BQ_M_SIMPLEX: the device table of the columns (k), their step states (k), their x, g, d, ub (k x sx_m each, in this order;
    // sx_m = n, or 2n for PAIRED), their labels (LABELS: k x n), their linear terms (k x sx_m, or null), the groups' tau (two groups:
    // k x 8), the offsets' results on the device (one r, two counts per group) and the groups' masses with bq_sx_check's `full`.  The
    // bq_solver of a column holds its scalars and records only
    bq_sx_col *sx_cols = nullptr;
    bq_sx_state *sx_state = nullptr;
    double *sx_vec = nullptr, *sx_sgn = nullptr, *sx_q = nullptr, *sx_tau = nullptr, *sx_rho = nullptr;
    long long *sx_counts = nullptr;
    std::vector<double> sx_mass;
    std::vector<int> sx_full;
    std::vector<long long> sx_ranges;   // BLOCKS: k x 4, the row offset and length of group 0 (class b), then of group 1 (class a)
    int64_t sx_m = 0;
    int sx_layout = BQ_SX_ONE;
    bool sx_has_x0 = false;
    bool initialised = false, started = false;
};

// a solver of bq_msolver_create_svr_boxes / _create_boxes: what bq_msolver_svr_heldout / _svc_heldout may score
static inline bool bq_msolver_is_boxes(const bq_msolver *m, int structure) {
    return m->boxes && m->method == BQ_M_PGFW && m->product == BQ_MP_SYMM16 && m->p->structure == structure;
}

// the structure map: the product input of column e at row i from its point, y o x (BQ_SVC) or x+ - x- (BQ_SVR)
__device__ inline double bq_mcol_input(const bq_epilogue &e, long long i, bool svr) {
    return svr ? e.x[i] - e.x[e.n + i] : e.sgn[i] * e.x[i];
}
