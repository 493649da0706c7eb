// The scalar part of scipy.sparse.linalg.minres (Paige-Saunders; scipy 1.15.3, no shift, no preconditioner) ONCE: the Lanczos
// coefficients, the Givens rotation and the seven stopping tests in scipy's order.  Its three users own the vectors and differ
// there by design: minres_normal_kernel (one persistent workgroup), mr_beta_kernel / mr_update_kernel (many workgroups, the state
// in device memory; both bq_minres.hip) and minres_solve (bq_xstar.hip: the recurrence on the host between two kernels).
// An iteration is:   the user's Lanczos step gives alfa = v'A v and |r2|^2   ->   rotate()   ->   the user updates
// w = (v - oldeps w1 - delta w2) denom,  x += phi w   ->   stop(|x|^2).
// Plain C++ apart from the guarded qualifiers: tests/c/minres_rec_check.cpp wraps a dense host MINRES around it and holds that to
// scipy itself.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define BQ_MINRES_HD __host__ __device__
#else
#define BQ_MINRES_HD
#endif

struct bq_minres_rec {
    double beta1, oldb, beta, dbar, epsln, phibar, rhs1, rhs2, tnorm2, gmax, gmin, cs, sn;
    double alfa, oldeps, delta, denom, phi, root;   // what rotate() hands to the vector update and to stop()
    int istop;                                      // scipy's code; 0: go on

    // beta1^2 = |b|^2 (x0 = 0).  beta1 == 0: x = 0 is the solution and no iteration takes place
    BQ_MINRES_HD void start(double beta1_squared) {
        beta1 = beta1_squared > 0.0 ? sqrt(beta1_squared) : 0.0;
        oldb = 0.0;
        beta = beta1;
        dbar = 0.0;
        epsln = 0.0;
        phibar = beta1;
        rhs1 = beta1;
        rhs2 = 0.0;
        tnorm2 = 0.0;
        gmax = 0.0;
        gmin = 1.7976931348623157e308;
        cs = -1.0;
        sn = 0.0;
        alfa = oldeps = delta = denom = phi = root = 0.0;
        istop = 0;
    }

    // iteration itn (from 1): the Lanczos step gave alfa and the squared norm of the next Lanczos vector
    BQ_MINRES_HD void rotate(double alfa_new, double beta_squared, long long itn) {
        const double eps = 2.220446049250313e-16;
        alfa = alfa_new;
        oldb = beta;
        beta = sqrt(beta_squared);
        tnorm2 += alfa * alfa + oldb * oldb + beta * beta;
        if (itn == 1 && beta / beta1 <= 10.0 * eps) istop = -1;
        oldeps = epsln;
        delta = cs * dbar + sn * alfa;
        const double gbar = sn * dbar - cs * alfa;
        epsln = sn * beta;
        dbar = -cs * beta;
        root = hypot(gbar, dbar);
        double gamma = hypot(gbar, beta);
        gamma = fmax(gamma, eps);
        cs = gbar / gamma;
        sn = beta / gamma;
        phi = cs * phibar;
        phibar = sn * phibar;
        denom = 1.0 / gamma;
        gmax = fmax(gmax, gamma);
        gmin = fmin(gmin, gamma);
        const double z = rhs1 / gamma;
        rhs1 = rhs2 - delta * z;
        rhs2 = -epsln * z;
    }

    // after x += phi w: the stopping tests; returns istop
    BQ_MINRES_HD int stop(double xnorm_squared, long long itn, long long maxiter, double rtol) {
        const double eps = 2.220446049250313e-16;
        const double ynorm = sqrt(xnorm_squared);
        const double Anorm = sqrt(tnorm2);
        const double epsx = Anorm * ynorm * eps;
        const double rnorm = phibar;
        const double test1 = (ynorm == 0.0 || Anorm == 0.0) ? INFINITY : rnorm / (Anorm * ynorm);
        const double test2 = (Anorm == 0.0) ? INFINITY : root / Anorm;
        const double Acond = gmax / gmin;
        if (istop == 0) {
            const double t1 = 1.0 + test1, t2 = 1.0 + test2;
            if (t2 <= 1.0) istop = 2;
            if (t1 <= 1.0) istop = 1;
            if (itn >= maxiter) istop = 6;
            if (Acond >= 0.1 / eps) istop = 4;
            if (epsx >= beta1) istop = 3;
            if (test2 <= rtol) istop = 2;
            if (test1 <= rtol) istop = 1;
        }
        return istop;
    }
};
