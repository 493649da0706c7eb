// Augmented-Lagrangian dual driven by the first-order ("stochastic", full batch) update rules — SURVEY 8(f).3.
//
// Restates on the device, for a QP  min 1/2 x'Qx + q'x  s.t.  a'x = 0 (optional row), lb <= x <= ub (each optional):
//   constraints  c = [a'x; lb - x; x - ub]                         optiml/opti/constrained/_base.py:239-296, 317-325
//   value        L = f(x) + dual'c + rho/2 |[c_eq; max(c_in, 0)]|^2           :326-340
//   gradient     Qx + q + dual'AG + rho AG_act'(AG_act x - bh_act)            :374-404
//   callback     primal value, past_x                                         optiml/opti/_base.py:96-117
//   multipliers  dual += rho c(x_new), inequality part clipped at 0; 'optimal' when |d dual| + |d x| <= tol or
//                |c| <= tol                                                   optiml/opti/_base.py:129-146
//   loop + rules optiml/opti/unconstrained/stochastic/{gradient_descent,adam,amsgrad,adamax,adagrad,adadelta,
//                rmsprop}.py (minimize): [nesterov jump] -> evaluate -> callback -> epoch test -> rule step ->
//                momentum -> multiplier update / stop test -> iter += 1.
// [A; -I; I] is never formed: every row is a coordinate or the single dense row a.  One panel product Q x per
// iteration gives the value, the primal value and the gradient (the reference spends three).  All O(n) work and all
// reductions are redundant per rank in a fixed order; only the panel product is sharded.
//
// An iteration is THREE launches with ONE chain of sums (round 6; six launches and two chains in rounds 2-5: prep, tiles, slab
// reduction, finish, eval + decisions, update + decisions):
//   the tile kernel;
//   the kernel that closes the product (bq_epilogue.h, kind 2): Qx, the sums of this evaluation AND of the previous iteration's stop
//   test per 256-row block; its last block closes the previous iteration (multiplier of the equality row, stop tests, iter += 1)
//   and takes this one's value, record and epoch test;
//   al_update_kernel: one elementwise pass — gradient, rule step, momentum, x, the multipliers of the bound rows, the per-element
//   terms of the stop test (summed by the NEXT closing kernel) and the next product's input.
// al_flush_kernel closes the last iteration of a bq_solver_run (same sums, same tree: the bits do not depend on how the iterations
// are cut into runs).  BQ_SVR structure keeps a launch of its own for the product's input; Nesterov momentum moves x before the
// gradient is taken, so its iterations are closed at once (flush after every update: five launches).
#include <cmath>

#include "bq_al.h"
#include "bq_al_update.h"
#include "bq_epilogue.h"


// nesterov: x += momentum * previous step, before the gradient is taken (gradient_descent.py:78-81 and the like)
__global__ void al_jump_kernel(int64_t N, bq_al_vecs V, double mom_const, const bq_scal *sc) {
    if (sc->done) return;
    const double mom = al_sched(V.mom_sched, V.sched_len, sc->iter, mom_const);
    BQ_VEC_LOOP(i) {
        if (i < N) V.x[i] = V.x[i] + __dmul_rn(mom, V.step[i]);
    }
}

// The stand-alone closing kernel of an iteration's evaluation (bq_epilogue.h, kind 2) for the paths whose product has no closing
// kernel of its own to carry it (dense row-block panels, the one-rank streamed product, BQ_SYM_EXCHANGE=allreduce): one workgroup
// per 256 rows, the sums have the same bits whichever kernel closed the product.
__global__ __launch_bounds__(256) void finish_al_kernel(const double *__restrict__ sv, bq_epilogue epi) {
    if (epi.sc->done) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bq_al_pre pre = bq_al_epi_preload(epi, i, true, true);
    bq_al_epi_finish<true>(epi, blockIdx.x, gridDim.x, bq_al_epi_element(epi, pre, i, i < epi.n ? sv[i] : 0.0, true), gridDim.x);
}

// closes the iteration whose update has run but whose stop test is still pending (the end of a bq_solver_run; every iteration
// with Nesterov momentum): the sums of bq_al_epi_finish without an evaluation
__global__ __launch_bounds__(256) void al_flush_kernel(bq_epilogue epi) {
    if (epi.sc->done || !epi.sc->al_pending) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bq_al_pre pre = bq_al_epi_preload(epi, i, true, false);
    bq_al_epi_finish<false>(epi, blockIdx.x, gridDim.x, bq_al_epi_element(epi, pre, i, 0.0, false), gridDim.x);
}

// gradient, rule step, momentum, x update, multiplier update of the coordinate rows, and the per-element terms of the stop test at
// the new point (the next closing kernel, or al_flush_kernel, sums them, updates the equality multiplier and decides): one
// elementwise pass, an element per thread
// (al_update_body, bq_al_update.h: the batched solver's update kernel runs the same body per column)
__global__ __launch_bounds__(256) void al_update_kernel(int64_t N, int64_t ldN, bq_al_vecs V, bq_al_params prm, bq_scal *sc,
                                                        const double *__restrict__ sgn, double *__restrict__ w_out) {
    al_update_body(N, ldN, V, prm, sc, sgn, w_out);
}

bq_epilogue bq_al_epilogue(bq_solver *s) {
    bq_al_state *al = s->al;
    bq_problem *p = s->p;
    bq_epilogue epi = {};
    epi.structure = p->structure;
    epi.kind = 2;
    epi.n = p->n;
    epi.N = p->N;
    epi.diag_add = p->diag_add;
    epi.x = al->V.x;
    epi.q = al->V.q;
    epi.lb = al->V.lb;
    epi.ub = al->V.ub;
    epi.sgn = p->sgn;
    epi.Qd = al->V.Qx;
    epi.sc = s->sc;
    epi.part = s->partials;
    epi.stats = s->stats;
    epi.a = al->V.a;
    epi.llb = al->V.llb;
    epi.lub = al->V.lub;
    epi.chk = al->V.chk;
    epi.ldN = s->ldN;
    epi.rho = al->prm.rho;
    epi.tol = al->prm.tol;
    epi.epochs = al->prm.epochs;
    epi.has_rows = (al->V.a != nullptr || al->V.lb != nullptr || al->V.ub != nullptr) ? 1 : 0;
    return epi;
}

// the end of a bq_solver_run: the last update's stop test must not stay pending across the call (its record leaves with this run)
int bq_al_flush(bq_solver *s) {
    al_flush_kernel<<<(unsigned)((s->p->n + 255) / 256), 256, 0, s->p->ctx->stream>>>(bq_al_epilogue(s));
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

int bq_al_iterate(bq_solver *s) {
    bq_al_state *al = s->al;
    bq_problem *p = s->p;
    hipStream_t st = p->ctx->stream;
    const int *done = &s->sc->done;
    const bq_al_params &prm = al->prm;
    const bool nesterov = prm.momentum_type == BQ_MOM_NESTEROV;
    if (nesterov) al_jump_kernel<<<bq_vec_grid(s->ldN), BQ_VEC_BLOCK, 0, st>>>(s->N, al->V, prm.momentum, s->sc);
    // the product's input: x itself (BQ_PLAIN), what the previous update kernel left in p->w (BQ_SVC, nothing has moved x since),
    // else the structure map of x by a launch of its own
    const double *w = al->V.x;
    if (p->structure != BQ_PLAIN) {
        if (!al->w_ready) BQ_TRY(bq_launch_prep(p, al->V.x, done));
        w = p->w;
    }
    const bq_epilogue epi = bq_al_epilogue(s);
    bool fused = false;
    BQ_TRY(bq_panel_product(p, p->add_one, w, done, &epi, &fused));
    if (!fused) finish_al_kernel<<<(unsigned)((p->n + 255) / 256), 256, 0, st>>>(p->s, epi);
    double *w_out = (p->structure == BQ_SVC && !nesterov) ? p->w : nullptr;
    al_update_kernel<<<(unsigned)((s->N + 255) / 256), 256, 0, st>>>(s->N, s->ldN, al->V, prm, s->sc, p->sgn, w_out);
    al->w_ready = w_out != nullptr;
    // Nesterov's jump of the NEXT iteration moves x before its gradient is taken: whether that iteration takes place must be known
    // before the jump, so the iteration is closed here instead of inside the next closing kernel
    if (nesterov) al_flush_kernel<<<(unsigned)((p->n + 255) / 256), 256, 0, st>>>(epi);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}
