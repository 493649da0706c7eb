// The kernel map of the row-based SMO solvers on one inner product (bq_gram_image.h / bq_exp.h), ONE definition for the one-row
// fma-chain kernels of bq_rsmo.hip and the 16-row MFMA passes of bq_mrsmo.hip, and the dispatch over its instantiations.
// PARAMS carries gamma, coef0 and degree.
#pragma once
#include "bq_common.h"
#include "bq_gram_image.h"

template <int KIND, int DEG, typename PARAMS>
__device__ __forceinline__ double rsmo_map(const PARAMS &P, double dot, double a_r, double a_t, bool diag) {
    if (KIND == BQ_KERNEL_RBF) {
        double dist = -2.0 * dot;
        const double norms = a_r + a_t;   // commutative: K[r][t] and K[t][r] take the same path
        dist += norms;
        dist = fmax(dist, 0.0);
        if (diag) dist = 0.0;
        return bq_exp(-P.gamma * dist);
    } else if (KIND == BQ_KERNEL_POLY) {
        return bq_poly_map<DEG>(P.gamma * dot + P.coef0, P.degree);
    } else if (KIND == BQ_KERNEL_SIGMOID) {
        return tanh(P.gamma * dot + P.coef0);
    }
    return dot;
}

template <int K, int D>
struct rsmo_kind {
    static constexpr int kind = K, deg = D;
};
template <typename F>
static int rsmo_dispatch(const bq_problem *p, F f) {
    switch (p->kernel) {
    case BQ_KERNEL_LINEAR: f(rsmo_kind<BQ_KERNEL_LINEAR, 0>{}); return BQ_OK;
    case BQ_KERNEL_RBF: f(rsmo_kind<BQ_KERNEL_RBF, 0>{}); return BQ_OK;
    case BQ_KERNEL_SIGMOID: f(rsmo_kind<BQ_KERNEL_SIGMOID, 0>{}); return BQ_OK;
    case BQ_KERNEL_POLY:
        if (p->degree == 1) f(rsmo_kind<BQ_KERNEL_POLY, 1>{});
        else if (p->degree == 2) f(rsmo_kind<BQ_KERNEL_POLY, 2>{});
        else if (p->degree == 3) f(rsmo_kind<BQ_KERNEL_POLY, 3>{});
        else f(rsmo_kind<BQ_KERNEL_POLY, 0>{});
        return BQ_OK;
    default: break;
    }
    bq_set_error("bad argument: the row kernel is built for the kernels a streamed problem takes (linear, poly, rbf, sigmoid)");
    return BQ_ERR_BADARG;
}
