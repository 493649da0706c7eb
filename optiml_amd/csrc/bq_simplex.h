// What bq_msolver.hip needs of the capped-simplex solver's kernels (bq_simplex.hip).
#pragma once
#include "bq_common.h"

constexpr double BQ_SX_MAX_ABS = 0x1p1021;   // largest box and largest |V| the projection takes: the bracket's width stays finite
constexpr int BQ_SX_WINDOW = 10;   // values of f the nonmonotone acceptance looks back on

// device-resident state of a simplex column beside its bq_scal (iter, max_iter, eps = tol, f, status, done, the records' window)
struct bq_sx_state {
    double s, alpha, viol, gd, dd;   // the spectral step, the last step length, the violation at x, g'd and d'd of the direction
    double win[BQ_SX_WINDOW];
    int nwin, pad;
};

// one column as the kernels take it
struct bq_sx_col {
    long long n;
    double *x, *g, *d;
    const double *ub;
    double mass;
    int full;     // mass >= sum ub: the set is the single point ub
    int has_x0;   // x holds the caller's start point (else the start is P(0))
    bq_scal *sc;
    bq_sx_state *st;
    bq_iter_stat *stats;
};

// cols: device table of k columns; pos, nlive: as in bq_msolver.hip.  init: the start point and W[:, c] = x of every column
int bq_sx_launch_project(const bq_sx_col *cols, int k, const int *pos, double *W, int64_t ldw, bool init, hipStream_t st);
int bq_sx_launch_start(const bq_sx_col *cols, int k, const double *out, int64_t ldw, hipStream_t st);
int bq_sx_launch_close(const bq_sx_col *cols, int k, const int *pos, const double *out, int64_t ldw, hipStream_t st);
int bq_sx_launch_top(const bq_sx_col *cols, int k, int *pos, int *nlive, hipStream_t st);
int bq_sx_launch_offsets(const bq_sx_col *cols, int k, double *rho, long long *n_sv, long long *n_free, hipStream_t st);
// the host checks of k boxes (k x n, finite, >= 0) and masses (0 < mass <= sum of the box); full[c]: mass[c] is the whole box
int bq_sx_check(int k, int64_t n, const double *UB, const double *mass, int *full);
