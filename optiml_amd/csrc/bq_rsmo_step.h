// The scalar rules of the row-based SMO (bq_rsmo.hip), ONE definition for the device and for the host check
// (tests/c/rsmo_step_check.cpp, run by tests/test_rsmo_step_host.py): libsvm's Solver without shrinking (svm.cpp: select_working_set,
// the two-variable update of Solve, calculate_rho), restated on
//     min 1/2 a'Qa + p'a,  y'a = 0,  0 <= a_t <= C_t,   Q_st = y_s y_t K_st,
// plus the victim rule of the row cache; and, for the general entry (bq_rsmo_create_general; host check tests/c/rsmo_nu_step_check.cpp,
// restatement tests/smo_nu_reference.py), Solver_NU's selection, stop test and r1 / r2 and the victim rule with two slots to keep.
// No HIP types: plain C++ on doubles and integers.
//
// Rounding.  Every sum, product and quotient below is one correctly rounded operation and none is fused (the includer builds with
// contraction inside a statement at most, and each product here is a statement of its own): the NumPy restatement
// (tests/smo_rows_reference.py) has the same bits.  Multiplications by y = +-1 and by 2 are exact.
#pragma once

#ifndef BQ_RSMO_FN
#if defined(__HIPCC__)
#define BQ_RSMO_FN __host__ __device__ __forceinline__
#else
#define BQ_RSMO_FN static inline
#endif
#endif

#define BQ_RSMO_TAU 1e-12
#define BQ_RSMO_INF (__builtin_inf())

// ---- the sets --------------------------------------------------------------------------------------------------------------------
// I_up: y = +1 below its box, y = -1 above 0 (libsvm: !is_upper_bound / !is_lower_bound); I_low the mirror image
BQ_RSMO_FN bool bq_rsmo_in_up(double y, double a, double C) { return y > 0.0 ? a < C : a > 0.0; }
BQ_RSMO_FN bool bq_rsmo_in_low(double y, double a, double C) { return y > 0.0 ? a > 0.0 : a < C; }
// what i maximises over I_up (-y_t G_t) and what Gmax2 maximises over I_low (y_t G_t)
BQ_RSMO_FN double bq_rsmo_up_value(double y, double G) { return y > 0.0 ? -G : G; }
BQ_RSMO_FN double bq_rsmo_low_value(double y, double G) { return y > 0.0 ? G : -G; }

// a (value, index) candidate of an arg-max / arg-min scan; libsvm's `>=` / `<=` scans in ascending t keep the LARGER index of equal
// values, and so does every combine here — the result of a scan does not depend on how it was cut into pieces
struct bq_rsmo_pick {
    double v;
    long long idx;   // -1: none
};
BQ_RSMO_FN bool bq_rsmo_max_before(double va, long long ia, double vb, long long ib) {   // a wins the arg-max over b
    return ia >= 0 && (ib < 0 || va > vb || (va == vb && ia > ib));
}
BQ_RSMO_FN bool bq_rsmo_min_before(double va, long long ia, double vb, long long ib) {   // a wins the arg-min over b
    return ia >= 0 && (ib < 0 || va < vb || (va == vb && ia > ib));
}

// ---- WSS2 ------------------------------------------------------------------------------------------------------------------------
// QD_i + QD_t - 2 y_i y_t Q_it = QD_i + QD_t - 2 K_it in every branch of libsvm (Q_it = y_i y_t K_it); <= 0: TAU
BQ_RSMO_FN double bq_rsmo_quad_coef(double qd_i, double qd_t, double k_it) {
    double q = qd_i + qd_t;
    const double twice = 2.0 * k_it;
    q = q - twice;
    return q > 0.0 ? q : BQ_RSMO_TAU;
}
// the score of t as partner of i: -(grad_diff)^2 / quad_coef, grad_diff = Gmax + y_t G_t; *ok false when t in I_low is no candidate
// (grad_diff <= 0).  The caller has tested t in I_low.
BQ_RSMO_FN double bq_rsmo_score(double gmax, double y_t, double g_t, double qd_i, double qd_t, double k_it, bool *ok) {
    const double grad_diff = gmax + bq_rsmo_low_value(y_t, g_t);
    *ok = grad_diff > 0.0;
    if (!*ok) return BQ_RSMO_INF;
    const double sq = grad_diff * grad_diff;
    const double quad = bq_rsmo_quad_coef(qd_i, qd_t, k_it);
    const double r = sq / quad;
    return -r;
}
// libsvm's stop test on the maxima of the two scans
BQ_RSMO_FN bool bq_rsmo_stop(double gmax, double gmax2, double tol) {
    const double gap = gmax + gmax2;
    return gap < tol;
}

// ---- the two-variable update, both clipping cascades in libsvm's order -----------------------------------------------------------------
// in: the pair's labels, gradients, boxes, diagonals and K_ij; in / out: the two multipliers
BQ_RSMO_FN void bq_rsmo_pair_update(double y_i, double y_j, double G_i, double G_j, double qd_i, double qd_j, double k_ij, double C_i,
                                    double C_j, double *alpha_i, double *alpha_j) {
    double ai = *alpha_i, aj = *alpha_j;
    const double quad = bq_rsmo_quad_coef(qd_i, qd_j, k_ij);
    if (y_i != y_j) {
        const double num = -G_i - G_j;
        const double delta = num / quad;
        const double diff = ai - aj;
        ai = ai + delta;
        aj = aj + delta;
        if (diff > 0.0) {
            if (aj < 0.0) {
                aj = 0.0;
                ai = diff;
            }
        } else {
            if (ai < 0.0) {
                ai = 0.0;
                aj = -diff;
            }
        }
        if (diff > C_i - C_j) {
            if (ai > C_i) {
                ai = C_i;
                aj = C_i - diff;
            }
        } else {
            if (aj > C_j) {
                aj = C_j;
                ai = C_j + diff;
            }
        }
    } else {
        const double num = G_i - G_j;
        const double delta = num / quad;
        const double sum = ai + aj;
        ai = ai - delta;
        aj = aj + delta;
        if (sum > C_i) {
            if (ai > C_i) {
                ai = C_i;
                aj = sum - C_i;
            }
        } else {
            if (aj < 0.0) {
                aj = 0.0;
                ai = sum;
            }
        }
        if (sum > C_j) {
            if (aj > C_j) {
                aj = C_j;
                ai = sum - C_j;
            }
        } else {
            if (ai < 0.0) {
                ai = 0.0;
                aj = sum;
            }
        }
    }
    *alpha_i = ai;
    *alpha_j = aj;
}

// G_t += Q_it d_i + Q_jt d_j: two rounded products, their rounded sum, one rounded add
BQ_RSMO_FN double bq_rsmo_grad(double G_t, double Q_it, double d_i, double Q_jt, double d_j) {
    const double pi = Q_it * d_i;
    const double pj = Q_jt * d_j;
    const double both = pi + pj;
    return G_t + both;
}

// ---- rho ---------------------------------------------------------------------------------------------------------------------------
// calculate_rho in ascending t: the mean of y_t G_t over the free variables, else the midpoint of the two bounds
struct bq_rsmo_rho {
    double ub = BQ_RSMO_INF, lb = -BQ_RSMO_INF, sum_free = 0.0;
    long long nr_free = 0;
};
BQ_RSMO_FN void bq_rsmo_rho_add(bq_rsmo_rho *r, double y, double a, double C, double G) {
    const double yG = y > 0.0 ? G : -G;
    if (a >= C) {
        if (y < 0.0)
            r->ub = yG < r->ub ? yG : r->ub;
        else
            r->lb = yG > r->lb ? yG : r->lb;
    } else if (a <= 0.0) {
        if (y > 0.0)
            r->ub = yG < r->ub ? yG : r->ub;
        else
            r->lb = yG > r->lb ? yG : r->lb;
    } else {
        r->nr_free += 1;
        r->sum_free = r->sum_free + yG;
    }
}
BQ_RSMO_FN double bq_rsmo_rho_value(const bq_rsmo_rho *r) {
    if (r->nr_free > 0) return r->sum_free / (double)r->nr_free;
    const double both = r->ub + r->lb;
    return both / 2.0;
}

// ---- Solver_NU (svm.cpp: Solver_NU::select_working_set, Solver_NU::calculate_rho) -----------------------------------------------------
// The nu-duals keep a second equality (each sign's mass), so a pair never crosses the signs.  libsvm scans each sign on its own, and
// within one sign its sets and values are the ones above: `ip` is the arg-max of -G over y = +1 with a < C and `in` the arg-max of G
// over y = -1 with a > 0 (bq_rsmo_in_up / bq_rsmo_up_value on one sign), Gmaxp2 / Gmaxn2 the maxima of G over y = +1 with a > 0 and
// of -G over y = -1 with a < C (bq_rsmo_in_low / bq_rsmo_low_value on one sign).  A candidate j is scored against the row of its own
// sign: grad_diff = Gmaxp + G_j (y_j = +1) or Gmaxn - G_j (y_j = -1), and y_i = y_j, so QD_i + QD_j - 2 Q_ij is bq_rsmo_quad_coef.
// A side without a maximal violator has Gmax = -inf and index -1: grad_diff = -inf, no candidate.
BQ_RSMO_FN double bq_rsmo_nu_score(double y_t, double g_t, double gmaxp, double qd_ip, double k_ip_t, double gmaxn, double qd_in,
                                   double k_in_t, double qd_t, bool *ok) {
    if (y_t > 0.0) return bq_rsmo_score(gmaxp, y_t, g_t, qd_ip, qd_t, k_ip_t, ok);
    return bq_rsmo_score(gmaxn, y_t, g_t, qd_in, qd_t, k_in_t, ok);
}
// the two sums of the stop test and the test: max(Gmaxp + Gmaxp2, Gmaxn + Gmaxn2) < tol
BQ_RSMO_FN double bq_rsmo_nu_gap(double gmax, double gmax2) { return gmax + gmax2; }
BQ_RSMO_FN bool bq_rsmo_nu_stop(double gmaxp, double gmaxp2, double gmaxn, double gmaxn2, double tol) {
    const double gp = bq_rsmo_nu_gap(gmaxp, gmaxp2);
    const double gn = bq_rsmo_nu_gap(gmaxn, gmaxn2);
    const double worst = gp > gn ? gp : gn;
    return worst < tol;
}
// calculate_rho in ascending t, one set of pieces per sign, on G itself (not y G): r1 over y = +1, r2 over y = -1
struct bq_rsmo_nu_rho {
    double ub[2] = {BQ_RSMO_INF, BQ_RSMO_INF}, lb[2] = {-BQ_RSMO_INF, -BQ_RSMO_INF}, sum_free[2] = {0.0, 0.0};
    long long nr_free[2] = {0, 0};
};
BQ_RSMO_FN void bq_rsmo_nu_rho_add(bq_rsmo_nu_rho *r, double y, double a, double C, double G) {
    const int s = y > 0.0 ? 0 : 1;
    if (a >= C) {
        r->lb[s] = G > r->lb[s] ? G : r->lb[s];
    } else if (a <= 0.0) {
        r->ub[s] = G < r->ub[s] ? G : r->ub[s];
    } else {
        r->nr_free[s] += 1;
        r->sum_free[s] = r->sum_free[s] + G;
    }
}
BQ_RSMO_FN double bq_rsmo_nu_rho_side(const bq_rsmo_nu_rho *r, int s) {
    if (r->nr_free[s] > 0) return r->sum_free[s] / (double)r->nr_free[s];
    const double both = r->ub[s] + r->lb[s];
    return both / 2.0;
}
// rho = (r1 - r2) / 2, r = (r1 + r2) / 2
BQ_RSMO_FN void bq_rsmo_nu_rho_value(const bq_rsmo_nu_rho *r, double *rho, double *rr) {
    const double r1 = bq_rsmo_nu_rho_side(r, 0), r2 = bq_rsmo_nu_rho_side(r, 1);
    const double diff = r1 - r2;
    const double sum = r1 + r2;
    *rho = diff / 2.0;
    *rr = sum / 2.0;
}

// ---- the row cache -------------------------------------------------------------------------------------------------------------------
// The victim of a miss: the slot with the smallest stamp (0: never used), the lower slot among equals, never `keep` (the slot of the
// other row of the pair in hand; -1: none).  slot a goes before slot b:
BQ_RSMO_FN bool bq_rsmo_victim_before(long long stamp_a, long long a, long long stamp_b, long long b) {
    return a >= 0 && (b < 0 || stamp_a < stamp_b || (stamp_a == stamp_b && a < b));
}
BQ_RSMO_FN long long bq_rsmo_victim(const long long *stamp, long long R, long long keep) {
    long long best = -1;
    for (long long s = 0; s < R; ++s)
        if (s != keep && bq_rsmo_victim_before(stamp[s], s, best < 0 ? 0 : stamp[best], best)) best = s;
    return best;
}
// the same with two slots to keep (a Solver_NU step holds the rows of ip and in while it resolves the row of j); -1: none
BQ_RSMO_FN long long bq_rsmo_victim2(const long long *stamp, long long R, long long keep_a, long long keep_b) {
    long long best = -1;
    for (long long s = 0; s < R; ++s)
        if (s != keep_a && s != keep_b && bq_rsmo_victim_before(stamp[s], s, best < 0 ? 0 : stamp[best], best)) best = s;
    return best;
}
