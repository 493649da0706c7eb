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

// a column's layout: bcqp.h's BQ_SX_LABELS and BQ_SX_PAIRED (two groups), the one-group column of bq_msolver_create_simplex, and the
// two-group column of bq_msolver_create_simplex2_pairs, whose groups are two row ranges of a class-sorted panel
enum { BQ_SX_ONE = 2, BQ_SX_BLOCKS = 3 };

// one column as the kernels take it: min 1/2 b'Kb + q'x over the product of its capped simplices, group t being {0 <= x <= ub on its
// rows, sum x = mass[t]}, with b = sum_j s_j x_j scattered to panel row j mod n.  ONE: m = n variables in one group, s = 1, q = 0 (the
// nu-one-class dual; sgn, q, tau null, mass[1] and full[1] unused).  LABELS: m = n, s = sgn, group 0 the rows with sgn = +1.  PAIRED:
// m = 2n, s = +1 on j < n (group 0) and -1 on j >= n (group 1).  BLOCKS: m = n, the column of pair (a, b), a < b, of a class-sorted
// panel: group t is the rows [goff[t], goff[t] + glen[t]), group 0 class b's with s = +1, group 1 class a's with s = -1 (a class's
// ghost rows have ub = 0); sgn and q null; no kernel reads or writes a row outside the two ranges
struct bq_sx_col {
    long long n, m;      // panel rows; variables
    double *x, *g, *d;   // m
    const double *ub;    // m
    const double *sgn;   // LABELS: n, exactly +-1 (+1 where ub = 0: such a row has no box in either group); else null
    const double *q;     // m, or null (0)
    double mass[2];
    int full[2];         // mass[t] >= the sum of group t's box: the set is the single point ub
    int has_x0;          // x holds the caller's start point (else the start is P(0) per group)
    double *tau;         // 8: the two groups' tau (lo, hi, th, tl each), from the search's workgroups to the direction pass
    long long goff[2], glen[2];   // BLOCKS: the groups' row ranges (goff[1] + glen[1] <= goff[0]); else 0
    bq_scal *sc;
    bq_sx_state *st;
    bq_iter_stat *stats;
};

// cols: device table of k columns of one layout; pos, nlive: as in bq_msolver.hip.  project: the search (two groups: one workgroup per
// (column, group), a launch of its own; ONE: inside the direction pass) and the direction pass; init: the start point and
// W[:, c] = the signed, folded x of every column.  offsets: libsvm's calculate_rho per group, r / n_sv / n_free: k, or k x 2
int bq_sx_launch_project(const bq_sx_col *cols, int k, int layout, const int *pos, double *W, int64_t ldw, bool init, hipStream_t st);
int bq_sx_launch_start(const bq_sx_col *cols, int k, int layout, const double *out, int64_t ldw, hipStream_t st);
int bq_sx_launch_close(const bq_sx_col *cols, int k, int layout, const int *pos, const double *out, int64_t ldw, hipStream_t st);
// top: pos null: the records and the stop tests only (the routed product keeps pos[] the identity; its plan numbers the live pairs)
int bq_sx_launch_top(const bq_sx_col *cols, int k, int *pos, int *nlive, hipStream_t st);
int bq_sx_launch_offsets(const bq_sx_col *cols, int k, int layout, double *r, long long *n_sv, long long *n_free, hipStream_t st);
// the host checks of k boxes (k x n, finite, >= 0) and masses (0 < mass <= sum of the box); full[c]: mass[c] is the whole box
int bq_sx_check(int k, int64_t n, const double *UB, const double *mass, int *full);
