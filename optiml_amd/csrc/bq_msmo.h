// What a scorer may read of a batched SMO solver (bq_smo.hip owns `bq_msmo`; bq_mscore.hip: bq_msmo_vote_heldout, _svr_heldout,
// _svc_heldout).  The walkers'
// per-column record and a read-only view of the solver: device pointers to the state the walkers leave, host copies of what the
// argument checks need.  Nothing here changes the solver.
#pragma once
#include "bq_common.h"

struct bq_smo_scal {
    double b_up, b_low;
    long long i_up, i_low;
    long long outer, steps, changed;
    int sweep_all, finished, err_flag, pad;
};

struct bq_msmo;

struct bq_msmo_view {
    bq_problem *p;
    int task, k;
    int64_t n;
    const double *Y, *A;         // device, k x n: labels (BQ_SVC) / targets, multipliers (BQ_SVR: alpha+)
    const double *AM;            // device, k x n, BQ_SVR: alpha-; null for BQ_SVC
    const bq_smo_scal *sc;       // device, k
    const int64_t *row_ptr;      // host, k + 1 offsets into rows / sign; null: the columns carry no row lists
    const int *rows;             // host: the columns' ascending row lists
    const signed char *sign;     // host, BQ_SVC with lists: the column's label (+1 / -1) on every listed row, in list order
};

bq_msmo_view bq_msmo_view_of(const bq_msmo *s);
