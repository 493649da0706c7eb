// The elementwise pass of an augmented-Lagrangian iteration (bq_al.hip), shared by the single solver's al_update_kernel and the
// batched solver's mal_update_kernel (bq_msolver.hip): ONE copy of the body, a column of the batch is an ordinary AL bq_solver.
#pragma once
#include "bq_common.h"
#include "bq_reduce.h"

// value of a schedule at the current iteration (the last entry continues), or the constant
__device__ __forceinline__ double al_sched(const double *sched, long long len, long long it, double constant) {
    return sched != nullptr ? sched[it < len ? it : len - 1] : constant;
}

// gradient, rule step, momentum, x update, multiplier update of the coordinate rows, and the per-element terms of the stop test at
// the new point (the next closing kernel, or al_flush_kernel, sums them, updates the equality multiplier and decides): one
// elementwise pass, an element per thread.  Called by every thread of a grid whose x dimension covers the N elements of ONE solver
// (its gridDim.x blocks of 256 take the al_last ticket; the batched kernel's y dimension is the column).
// w_out (BQ_SVC without Nesterov momentum): the next product's input y o x_new, so that no prep launch precedes the tile kernel
__device__ __forceinline__ void al_update_body(int64_t N, int64_t ldN, bq_al_vecs V, bq_al_params prm, bq_scal *sc,
                                               const double *__restrict__ sgn, double *__restrict__ w_out) {
    const bool last = sc->al_last != 0;   // 'stopped' at this evaluation: write its gradient, take no step
    if (sc->done && !last) return;
    const double ax = sc->al_ax, mu = sc->al_mu, rho = prm.rho;
    const double lr = al_sched(V.lr_sched, V.sched_len, sc->iter, prm.step_size);
    const double mom = al_sched(V.mom_sched, V.sched_len, sc->iter, prm.momentum);
    const bool eq_act = V.a != nullptr && ax != 0.0;
    const double t = (double)(sc->iter + 1);
    double c1 = 1.0, c2 = 1.0;   // bias corrections 1 - beta^t
    if (prm.rule == BQ_RULE_ADAM || prm.rule == BQ_RULE_ADAMAX) c1 = 1.0 - pow(prm.beta1, t);
    if (prm.rule == BQ_RULE_ADAM) c2 = 1.0 - pow(prm.beta2, t);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) {
        const double x = V.x[i];
        // ---- gradient at x -------------------------------------------------------------------------------
        double g = V.Qx[i] + V.q[i];
        double dual_ag = 0.0, t3 = 0.0, t4 = 0.0;
        if (V.a) {
            dual_ag = __dmul_rn(mu, V.a[i]);
            if (eq_act) t3 = __dmul_rn(V.a[i], ax);
        }
        if (V.lb) {
            dual_ag -= V.llb[i];
            if (V.lb[i] - x > 0.0) {
                t3 += x;
                t4 += V.lb[i];
            }
        }
        if (V.ub) {
            dual_ag += V.lub[i];
            if (x - V.ub[i] > 0.0) {
                t3 += x;
                t4 += V.ub[i];
            }
        }
        g = ((g + dual_ag) + __dmul_rn(rho, t3)) - __dmul_rn(rho, t4);
        V.g[i] = g;
        V.xe[i] = x;
        if (!last) {
            // ---- rule step -----------------------------------------------------------------------------------
            const double d = -g, g2 = __dmul_rn(g, g);
            double s;
            switch (prm.rule) {
                case BQ_RULE_ADAM: {
                    const double m = __dmul_rn(prm.beta1, V.s1[i]) + __dmul_rn(1.0 - prm.beta1, d);
                    const double v = __dmul_rn(prm.beta2, V.s2[i]) + __dmul_rn(1.0 - prm.beta2, g2);
                    V.s1[i] = m;
                    V.s2[i] = v;
                    s = __dmul_rn(lr, m / c1) / (sqrt(v / c2) + prm.offset);
                    break;
                }
                case BQ_RULE_AMSGRAD: {
                    const double m = __dmul_rn(prm.beta1, V.s1[i]) + __dmul_rn(1.0 - prm.beta1, d);
                    const double v = __dmul_rn(prm.beta2, V.s2[i]) + __dmul_rn(1.0 - prm.beta2, g2);
                    const double vm = fmax(v, V.s3[i]);
                    V.s1[i] = m;
                    V.s2[i] = v;
                    V.s3[i] = vm;
                    s = __dmul_rn(lr, m) / (sqrt(vm) + prm.offset);
                    break;
                }
                case BQ_RULE_ADAMAX: {
                    const double m = __dmul_rn(prm.beta1, V.s1[i]) + __dmul_rn(1.0 - prm.beta1, d);
                    const double u = fmax(__dmul_rn(prm.beta2, V.s2[i]), fabs(g));
                    V.s1[i] = m;
                    V.s2[i] = u;
                    s = __dmul_rn(lr, m / c1) / (u + prm.offset);
                    break;
                }
                case BQ_RULE_ADAGRAD: {
                    const double acc = V.s1[i] + g2;
                    V.s1[i] = acc;
                    s = __dmul_rn(lr, d) / sqrt(acc + prm.offset);
                    break;
                }
                case BQ_RULE_ADADELTA: {
                    const double acc = __dmul_rn(prm.decay, V.s1[i]) + __dmul_rn(1.0 - prm.decay, g2);
                    V.s1[i] = acc;
                    s = __dmul_rn(__dmul_rn(lr, d), sqrt(V.s2[i] + prm.offset) / sqrt(acc + prm.offset));
                    break;
                }
                case BQ_RULE_RMSPROP: {
                    const double acc = __dmul_rn(prm.decay, V.s1[i]) + __dmul_rn(1.0 - prm.decay, g2);
                    V.s1[i] = acc;
                    s = __dmul_rn(lr, d) / sqrt(acc + prm.offset);
                    break;
                }
                default: s = __dmul_rn(lr, d); break;   // BQ_RULE_SGD
            }
            // ---- momentum: step = momentum * previous step + s in both variants; nesterov already moved x by the
            // first term before the gradient was taken ------------------------------------------------------------
            double step = s, xn;
            if (prm.momentum_type == BQ_MOM_POLYAK) {
                step = __dmul_rn(mom, V.step[i]) + s;
                xn = x + step;
            } else if (prm.momentum_type == BQ_MOM_NESTEROV) {
                step = __dmul_rn(mom, V.step[i]) + s;
                xn = x + s;
            } else {
                xn = x + step;
            }
            V.step[i] = step;
            V.x[i] = xn;
            if (w_out != nullptr) w_out[i] = sgn[i] * xn;
            if (prm.rule == BQ_RULE_ADADELTA)   // adadelta.py:122 (only reached when the stop test fails: a stop ends the solve anyway)
                V.s2[i] = __dmul_rn(prm.decay, V.s2[i]) + __dmul_rn(1.0 - prm.decay, __dmul_rn(step, step));
            // ---- constraints at the new point, multiplier update of the coordinate rows --------------------------
            double cn = 0.0, dl = 0.0;
            if (V.lb) {
                const double c = V.lb[i] - xn, old = V.llb[i];
                const double nw = fmax(old + __dmul_rn(rho, c), 0.0);
                V.llb[i] = nw;
                cn += c * c;
                dl += (nw - old) * (nw - old);
            }
            if (V.ub) {
                const double c = xn - V.ub[i], old = V.lub[i];
                const double nw = fmax(old + __dmul_rn(rho, c), 0.0);
                V.lub[i] = nw;
                cn += c * c;
                dl += (nw - old) * (nw - old);
            }
            V.chk[i] = cn;
            V.chk[ldN + i] = dl;
            V.chk[2 * ldN + i] = (xn - x) * (xn - x);
        }
    }
    if (last) {   // uniform: no step after the last evaluation; the flag is consumed by the block that finishes last
        if (bq_last_block(&sc->ticket[1], gridDim.x) && threadIdx.x == 0) sc->al_last = 0;
        return;
    }
    if (i == 0) sc->al_pending = 1;   // read by the NEXT kernel (the closing kernel of the next product, or al_flush_kernel)
}
