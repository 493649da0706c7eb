// One entry H[i][j] of the Hessian a factorisation works on, read from a problem's resident panel (the H assembly of the
// factorisations and the ActiveSet update columns share it): dense panels as stored, kernel panels through the structure flags
// (BQ_SVC: y_i y_j (K_ij + 1), BQ_SVR: +-(K + 1) on the n x n blocks, BQ_H_KPLUS1: K + 1), plus diag_add on the diagonal.
//
// H is symmetric by construction — ONE triangle of the panel is read and mirrored, as LAPACK's potrf does:
//   packed != 0  packed lower tile rows (kernel-built panels, a dense Q == Q', BQ_DENSE_LOWER): the tiles on/below the diagonal
//                are all there is, element (max, min) at bq_sym_addr
//   packed == 0  whole rows of pitch ldp (BQ_DENSE_ROWS, any dense Q that is not symmetric, BQ_FULL_PANEL): the UPPER triangle,
//                element (min, max) at min * ldp + max — what scipy's cho_factor (lower=False) reads of the reference's Q
//                (optiml/opti/_base.py:263, constrained/active_set.py:141, interior_point.py:235)
#pragma once
#include "bq_c7.h"
#include "bq_common.h"

constexpr int BQ_H_KPLUS1_MODE = 3;   // == BQ_H_KPLUS1 (bq_chol.h)

// where panel element (r, c) of an n x n panel and its mirror image (c, r) are read
__device__ __forceinline__ int64_t bq_q_addr(int64_t ldp, int packed, int64_t r, int64_t c) {
    const int64_t hi = r > c ? r : c, lo = r > c ? c : r;
    return packed ? bq_sym_addr(hi, lo, 0) : lo * ldp + hi;
}

template <typename P>   // P: const double *, const float * or the compact layout's bq_c7p (bq_c7.h)
__device__ __forceinline__ double bq_q_elem(int structure, P panel, int64_t ldp, int packed, int64_t n,
                                            const double *__restrict__ sgn, double diag_add, int64_t i, int64_t jj) {
    double v;
    if (structure == BQ_PLAIN) {
        v = (double)panel[bq_q_addr(ldp, packed, i, jj)];
    } else if (structure == BQ_SVC) {
        v = sgn[i] * sgn[jj] * ((double)panel[bq_q_addr(ldp, packed, i, jj)] + 1.0);
    } else if (structure == BQ_H_KPLUS1_MODE) {
        v = (double)panel[bq_q_addr(ldp, packed, i, jj)] + 1.0;
    } else {
        const int64_t ii = i >= n ? i - n : i, jn = jj >= n ? jj - n : jj;
        const double pv = (double)panel[bq_q_addr(ldp, packed, ii, jn)] + 1.0;
        v = ((i >= n) == (jj >= n)) ? pv : -pv;
    }
    if (i == jj && diag_add != 0.0) v += diag_add;
    return v;
}
