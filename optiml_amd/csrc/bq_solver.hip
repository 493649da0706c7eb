// The single-problem solvers' C ABI (bcqp.h): creation and destruction of ProjectedGradient / FrankWolfe / ActiveSet / InteriorPoint and
// augmented-Lagrangian solvers, bq_solver_run's host loop, the read-outs, checkpoint / resume.  The iterations themselves live next
// to their kernels (bq_vec.hip, bq_as.hip, bq_ip.hip, bq_al.hip).
#include <algorithm>
#include <cmath>

#include "bq_al.h"

// ---------------------------------------------------------------------------------------------
// solvers
// ---------------------------------------------------------------------------------------------
static int alloc_vec(bq_solver *s, double **v) {
    BQ_HIP_CHAIN(bq_dev_zeroed(hipSuccess, s->mem, v, s->ldN, s->p->ctx->stream), "allocating a solver vector");
    return BQ_OK;
}

extern "C" int bq_solver_destroy(bq_solver *s) {
    if (s == nullptr) return BQ_OK;
    hipSetDevice(s->p->ctx->device);
    (void)bq_ctx_sync(s->p->ctx);   // may sit behind a collective: bounded when a collective timeout is set
    if (s->chol) bq_chol_ws_destroy(s->chol);
    if (s->flag_host) {
        hipHostFree(s->flag_host);
        hipEventDestroy(s->flag_event);
    }
    bq_as_free(s);
    delete s->resume;
    delete s->al;
    bq_problem *p = s->p;
    delete s;   // s->mem frees the device buffers
    // the solve the placement choice was made for is over: what it held back to keep this solve undisturbed can go now (bq_ctx::held)
    bq_ctx_release_held(p->ctx, p);
    bq_problem_unref(p);
    return BQ_OK;
}

extern "C" int bq_solver_create(bq_problem *p, int kind, const double *lb, const double *ub, const double *x0,
                                double eps, int64_t max_iter, double fw_t, bq_solver **out) {
    BQ_ARG(p && ub && out, "NULL argument");
    BQ_ARG(kind == BQ_PG || kind == BQ_FW || kind == BQ_AS || kind == BQ_IP || kind == BQ_AS_CG, "solver kind");
    const bool as_cg = kind == BQ_AS_CG;   // ActiveSet on products only: none of the dense-factor restrictions below
    if (as_cg) kind = BQ_AS;
    BQ_ARG(max_iter > 0, "max_iter must be > 0");             // optiml/opti/_base.py:73-74
    BQ_ARG(fw_t >= 0.0 && fw_t < 1.0, "t has to lie in [0, 1)");  // frank_wolfe.py:84-85
    if ((kind == BQ_IP || kind == BQ_AS) && !as_cg && p->ctx->world > 1) {
        bq_set_error("InteriorPoint/ActiveSet factorise the whole Hessian: use a single-rank context (replicas only)");
        return BQ_ERR_BADARG;
    }
    if ((kind == BQ_IP || kind == BQ_AS) && !as_cg && p->streamed) {
        bq_set_error("InteriorPoint/ActiveSet assemble their systems from the resident panel: not available in the streamed mode");
        return BQ_ERR_BADARG;
    }
    if ((kind == BQ_IP || kind == BQ_AS) && p->structure != BQ_PLAIN && !p->add_one) {
        bq_set_error("InteriorPoint/ActiveSet are not built for the BQ_NO_RANK_ONE duals (svm/_base.py:621-624)");
        return BQ_ERR_BADARG;
    }
    bq_ctx *c = p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    bq_solver *s = new bq_solver();
    s->p = p;
    p->refs += 1;
    s->kind = kind;
    s->as_cg = as_cg;
    s->N = p->N;
    s->ldN = p->ldN;
    s->nblk = p->ldN / BQ_VEC_TILE;
    int rc = BQ_OK;
    for (double **v : {&s->x, &s->g, &s->d, &s->Qd, &s->lb, &s->ub})
        if (rc == BQ_OK) rc = alloc_vec(s, v);
    if (rc == BQ_OK && kind == BQ_IP)
        for (double **v : {&s->lp, &s->lm, &s->rhs, &s->hd, &s->dlp, &s->dlm})
            if (rc == BQ_OK) rc = alloc_vec(s, v);
    if (rc != BQ_OK) {
        bq_solver_destroy(s);
        return rc;
    }
    std::vector<double> h((size_t)s->N);
    auto up = [&](double *dev, const double *src) {
        return hipMemcpyAsync(dev, src, sizeof(double) * s->N, hipMemcpyHostToDevice, c->stream);
    };
    hipError_t e = up(s->ub, ub);
    if (e == hipSuccess && lb) e = up(s->lb, lb);
    if (e == hipSuccess) {
        if (x0) {
            e = up(s->x, x0);
        } else {
            for (int64_t i = 0; i < s->N; ++i) h[i] = ((lb ? lb[i] : 0.0) + ub[i]) / 2;  // constrained/_base.py:65
            e = up(s->x, h.data());
        }
    }
    if (e == hipSuccess) e = s->mem.dev(&s->partials, BQ_MAX_PARTIAL_Q * s->nblk);
    if (e == hipSuccess) e = s->mem.dev(&s->sc, 1);
    if (e == hipSuccess) {
        memset(&s->host, 0, sizeof(bq_scal));
        s->host.max_iter = max_iter;
        s->host.eps = eps;
        s->host.fw_t = fw_t;
        s->host.status = BQ_STATUS_UNKNOWN;
        s->host.best_lb = -INFINITY;
        s->host.f = NAN;
        e = hipMemcpyAsync(s->sc, &s->host, sizeof(bq_scal), hipMemcpyHostToDevice, c->stream);
    }
    if (e == hipSuccess) {   // may sit behind a collective of an earlier solve: the bounded wait
        const int src = bq_ctx_sync(c);
        if (src != BQ_OK) {
            bq_solver_destroy(s);
            return src;
        }
    }
    if (e != hipSuccess) {
        bq_set_error("solver setup failed: %s", hipGetErrorString(e));
        bq_solver_destroy(s);
        return BQ_ERR_HIP;
    }
    if (kind == BQ_PG || kind == BQ_FW) {   // their every iteration is one product with the rank-one term: the Hessian image (bq_h52.h)
        rc = bq_hessian_image_ensure(p);
        if (rc != BQ_OK) {
            bq_solver_destroy(s);
            return rc;
        }
    }
    if ((kind == BQ_IP || kind == BQ_AS) && !as_cg) {
        // InteriorPoint on the SVR structure factorises the reduced n x n system (bq_ip.hip)
        rc = bq_chol_ws_create(c, (kind == BQ_IP && p->structure == BQ_SVR && bq_ip_svr_reduced()) ? p->n : s->N,
                               &s->chol);
        if (rc != BQ_OK) {
            bq_solver_destroy(s);
            return rc;
        }
    }
    *out = s;
    return BQ_OK;
}

extern "C" int bq_solver_set_inner(bq_solver *s, double rtol, int64_t max_iter) {
    BQ_ARG(s, "NULL solver");
    BQ_ARG(s->kind == BQ_AS && s->as_cg, "only the conjugate-gradient ActiveSet (BQ_AS_CG) has an inner iteration");
    BQ_ARG(rtol > 0.0 && rtol < 1.0, "inner tolerance must lie in (0, 1)");
    BQ_ARG(max_iter >= 0, "inner iteration cap must be >= 0 (0: 2 |A| + 50)");
    s->inner_rtol = rtol;
    s->inner_max = max_iter;
    return BQ_OK;
}

extern "C" int bq_solver_inner_iters(bq_solver *s, int64_t *total) {
    BQ_ARG(s && total, "NULL argument");
    *total = s->kind == BQ_AS ? bq_as_inner_iters(s) : 0;
    return BQ_OK;
}

extern "C" int bq_solver_counter(bq_solver *s, int which, int64_t *value) {
    BQ_ARG(s && value, "NULL argument");
    BQ_ARG(which >= BQ_COUNT_INNER && which <= BQ_COUNT_NO_PRODUCT, "which: BQ_COUNT_*");
    *value = s->kind == BQ_AS ? bq_as_counter(s, which) : 0;
    return BQ_OK;
}

extern "C" int bq_al_solver_create(bq_problem *p, const bq_al_params *prm, const double *a_eq, const double *lb,
                                   const double *ub, const double *x0, const double *dual0, bq_solver **out) {
    BQ_ARG(p && prm && x0 && out, "NULL argument");
    BQ_ARG(prm->rule >= BQ_RULE_SGD && prm->rule <= BQ_RULE_RMSPROP, "update rule");
    BQ_ARG(prm->momentum_type >= BQ_MOM_NONE && prm->momentum_type <= BQ_MOM_NESTEROV, "unknown momentum type");
    BQ_ARG(prm->momentum_type == BQ_MOM_NONE || (prm->rule != BQ_RULE_ADAGRAD && prm->rule != BQ_RULE_ADADELTA),
           "AdaGrad / AdaDelta take no momentum");
    BQ_ARG(prm->step_size > 0.0, "step_size must be > 0");                       // stochastic/_base.py:86-87
    BQ_ARG(prm->momentum >= 0.0 && prm->momentum < 1.0, "momentum must be between 0 and 1");   // :240-241
    BQ_ARG(prm->epochs > 0, "max_iter must be > 0");                             // optiml/opti/_base.py:73-74
    BQ_ARG(prm->rho > 0.0, "rho must be must > 0");                              // constrained/_base.py:276-277
    BQ_ARG(prm->offset > 0.0 || prm->rule == BQ_RULE_SGD, "offset must be > 0");
    BQ_ARG(prm->beta1 >= 0.0 && prm->beta1 < 1.0, "beta1 has to lie in [0, 1)");
    BQ_ARG(prm->beta2 >= 0.0 && prm->beta2 < 1.0, "beta2 has to lie in [0, 1)");
    BQ_ARG(prm->decay >= 0.0 && prm->decay < 1.0, "decay has to lie in [0, 1)");
    bq_ctx *c = p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    bq_solver *s = new bq_solver();
    s->p = p;
    p->refs += 1;
    s->kind = BQ_AL;
    s->N = p->N;
    s->ldN = p->ldN;
    s->nblk = p->ldN / BQ_VEC_TILE;
    s->al = new bq_al_state();
    s->al->prm = *prm;
    bq_al_vecs &V = s->al->V;
    memset(&V, 0, sizeof(V));
    int rc = BQ_OK;
    for (double **v : {&s->x, &s->g, &s->d, &s->Qd, &V.xe, &V.s1})
        if (rc == BQ_OK) rc = alloc_vec(s, v);
    if (rc == BQ_OK && s->mem.dev(&V.chk, 3 * s->ldN) != hipSuccess) {
        bq_set_error("cannot allocate the solver's vectors");
        rc = BQ_ERR_NOMEM;
    }
    if (rc == BQ_OK) BQ_HIP(hipMemsetAsync(V.chk, 0, sizeof(double) * 3 * s->ldN, c->stream));
    const bool two = prm->rule == BQ_RULE_ADAM || prm->rule == BQ_RULE_AMSGRAD || prm->rule == BQ_RULE_ADAMAX ||
                     prm->rule == BQ_RULE_ADADELTA;
    if (rc == BQ_OK && two) rc = alloc_vec(s, &V.s2);
    if (rc == BQ_OK && prm->rule == BQ_RULE_AMSGRAD) rc = alloc_vec(s, &V.s3);
    if (rc == BQ_OK && a_eq) rc = alloc_vec(s, &V.a);
    if (rc == BQ_OK && lb) rc = alloc_vec(s, &s->lb);
    if (rc == BQ_OK && lb) rc = alloc_vec(s, &V.llb);
    if (rc == BQ_OK && ub) rc = alloc_vec(s, &s->ub);
    if (rc == BQ_OK && ub) rc = alloc_vec(s, &V.lub);
    if (rc != BQ_OK) {
        bq_solver_destroy(s);
        return rc;
    }
    V.x = s->x;
    V.g = s->g;
    V.step = s->d;
    V.Qx = s->Qd;
    V.q = p->q;
    V.lb = lb ? s->lb : nullptr;
    V.ub = ub ? s->ub : nullptr;
    auto up = [&](double *dev, const double *src) {
        return hipMemcpyAsync(dev, src, sizeof(double) * s->N, hipMemcpyHostToDevice, c->stream);
    };
    hipError_t e = up(s->x, x0);
    if (e == hipSuccess) e = up(V.xe, x0);
    if (e == hipSuccess && a_eq) e = up(V.a, a_eq);
    if (e == hipSuccess && lb) e = up(s->lb, lb);
    if (e == hipSuccess && ub) e = up(s->ub, ub);
    std::vector<double> ones;
    if (e == hipSuccess && prm->rule == BQ_RULE_RMSPROP) {   // rmsprop.py: moving_mean_squared starts at ones
        ones.assign((size_t)s->N, 1.0);
        e = up(V.s1, ones.data());
    }
    memset(&s->host, 0, sizeof(bq_scal));
    if (dual0) {
        const double *d0 = dual0;
        if (a_eq) s->host.al_mu = *d0++;
        if (e == hipSuccess && lb) {
            e = up(V.llb, d0);
            d0 += s->N;
        }
        if (e == hipSuccess && ub) e = up(V.lub, d0);
    }
    if (e == hipSuccess) e = s->mem.dev(&s->partials, BQ_MAX_PARTIAL_Q * s->nblk);
    if (e == hipSuccess) e = s->mem.dev(&s->sc, 1);
    if (e == hipSuccess) {
        s->host.max_iter = prm->epochs;
        s->host.eps = prm->tol;
        s->host.status = BQ_STATUS_UNKNOWN;
        s->host.f = NAN;
        s->host.al_pf = NAN;
        e = hipMemcpyAsync(s->sc, &s->host, sizeof(bq_scal), hipMemcpyHostToDevice, c->stream);
    }
    if (e == hipSuccess) {   // may sit behind a collective of an earlier solve: the bounded wait
        const int src = bq_ctx_sync(c);
        if (src != BQ_OK) {
            bq_solver_destroy(s);
            return src;
        }
    }
    if (e != hipSuccess) {
        bq_set_error("solver setup failed: %s", hipGetErrorString(e));
        bq_solver_destroy(s);
        return BQ_ERR_HIP;
    }
    *out = s;
    return BQ_OK;
}

extern "C" int bq_al_solver_set_schedules(bq_solver *s, const double *step_sizes, const double *momenta, int64_t count) {
    BQ_ARG(s != nullptr && s->al != nullptr, "not an augmented-Lagrangian solver");
    BQ_ARG(count >= 1 && (step_sizes || momenta), "count >= 1 and at least one schedule");
    BQ_ARG(!s->initialised && s->host.iter == 0, "schedules are set before the first run");
    bq_ctx *c = s->p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    for (int64_t i = 0; i < count; ++i) {
        BQ_ARG(!step_sizes || step_sizes[i] > 0.0, "step sizes must be > 0");
        BQ_ARG(!momenta || (momenta[i] >= 0.0 && momenta[i] < 1.0), "momentum must be between 0 and 1");
    }
    bq_al_vecs &V = s->al->V;
    for (int k = 0; k < 2; ++k) {
        const double *src = k == 0 ? step_sizes : momenta;
        if (!src) continue;
        double *dev = nullptr;
        BQ_HIP(s->mem.dev(&dev, count));
        BQ_HIP(hipMemcpy(dev, src, sizeof(double) * count, hipMemcpyHostToDevice));
        const double *&sched = k == 0 ? V.lr_sched : V.mom_sched;
        s->mem.release(sched);   // schedules set before: the new one is in place first, as ever
        sched = dev;
    }
    V.sched_len = count;
    return BQ_OK;
}

extern "C" int bq_al_solver_dual_size(const bq_solver *s, int64_t *n_dual) {
    BQ_ARG(s && n_dual, "NULL argument");
    BQ_ARG(s->al != nullptr, "not an augmented-Lagrangian solver");
    const bq_al_vecs &V = s->al->V;
    *n_dual = (V.a ? 1 : 0) + (V.llb ? s->N : 0) + (V.lub ? s->N : 0);
    return BQ_OK;
}

static int solver_first(bq_solver *s) {
    if (s->kind == BQ_AL) return BQ_OK;   // nothing to prepare: every iteration evaluates Q x afresh
    bq_solver::resume_t *r = s->resume;
    const int have = r ? r->have : 0;
    hipStream_t st = s->p->ctx->stream;
    auto up = [&](double *dev, const std::vector<double> &src) {
        return hipMemcpyAsync(dev, src.data(), sizeof(double) * s->N, hipMemcpyHostToDevice, st);
    };
    switch (s->kind) {
        case BQ_PG:
        case BQ_FW:
            // g given: the start product is not needed — (x, g) is the whole state of these two (bq_solver_set_state)
            if (have & BQ_STATE_G) BQ_HIP(up(s->g, r->g));
            else BQ_TRY(bq_pgfw_start(s));
            break;
        case BQ_IP:
            // interior_point.py:180-186 where something is missing; what was given then replaces what the start formed
            if ((have & (BQ_STATE_G | BQ_STATE_MULT)) != (BQ_STATE_G | BQ_STATE_MULT)) BQ_TRY(bq_ip_start(s));
            if (have & BQ_STATE_G) BQ_HIP(up(s->g, r->g));
            if (have & BQ_STATE_MULT) {
                BQ_HIP(up(s->lp, r->lp));
                BQ_HIP(up(s->lm, r->lm));
            }
            break;
        default:
            BQ_TRY(bq_as_start(s));   // takes the masks from s->resume itself (they are allocated there)
            if (have & BQ_STATE_G) BQ_HIP(up(s->g, r->g));
            break;
    }
    if (r) {
        BQ_SYNC(s->p->ctx);   // the uploads read the vectors about to be released
        delete r;
        s->resume = nullptr;
    }
    return BQ_OK;
}

static int solver_iterate(bq_solver *s) {
    if (s->kind == BQ_AL) return bq_al_iterate(s);
    switch (s->kind) {
        case BQ_PG:
        case BQ_FW:
            return bq_pgfw_iterate(s);
        case BQ_IP:
            return bq_ip_iterate(s);
        default:
            return bq_as_iterate(s);
    }
}

extern "C" int bq_solver_run(bq_solver *s, int64_t max_steps, bq_iter_stat *stats, int64_t stats_cap, int64_t *n_stats,
                             int *status) {
    BQ_ARG(s && n_stats && status, "NULL argument");
    BQ_ARG(max_steps > 0, "max_steps must be > 0");
    BQ_ARG(stats == nullptr || stats_cap >= max_steps, "stats capacity must be >= max_steps");
    bq_ctx *c = s->p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    *n_stats = 0;
    *status = s->host.status;
    if (s->host.done) return BQ_OK;
    if (s->stats_cap < max_steps) {
        s->mem.release(s->stats);
        BQ_HIP(s->mem.dev(&s->stats, max_steps));
        s->stats_cap = max_steps;
    }
    if (s->flag_host == nullptr) {   // pinned flag + event of the lagged done-flag polling (best effort)
        if (hipHostMalloc((void **)&s->flag_host, sizeof(int), hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&s->flag_event, hipEventDisableTiming) != hipSuccess) {
            if (s->flag_host) hipHostFree(s->flag_host);
            s->flag_host = nullptr;
            (void)hipGetLastError();
        } else {
            *s->flag_host = 0;
        }
    }
    if (s->al) s->al->w_ready = false;   // p->w belongs to the problem: anything may have used it since the last run
    const long long base = s->host.iter;
    long long hdr[2] = {base, (long long)max_steps};
    BQ_HIP(hipMemcpyAsync(&s->sc->stat_base, hdr, sizeof(hdr), hipMemcpyHostToDevice, c->stream));
    if (!s->initialised) {
        BQ_TRY(solver_first(s));
        s->initialised = true;
    }
    // How often the host looks at the device `done` flag: kernels early-exit on the flag, so a late look only costs a few
    // no-op launches (~20 us per skipped iteration).  The factorising solvers are host-enqueued O(n^3) work per iteration
    // and look every time; PG/FW look about every 20 ms of estimated panel streaming time.  A look is a 4-byte copy to the
    // host plus an event on the stream — not free between two short kernels: at 2 ms (round 3) BASELINE config 2 ran 0.3035 ms
    // per iteration, at 20 ms 0.286 ms (profiles/r04/share_gaps_events.txt).
    int64_t poll = 1;
    if (s->kind == BQ_PG || s->kind == BQ_FW || s->kind == BQ_AL) {
        // The interval must be the SAME on every rank (each iteration contains a collective: ranks that stopped enqueueing at
        // different iterations would leave the others inside it), so it is computed from the mean share n / world, not from
        // this rank's own rows.
        const double esz = s->p->storage == BQ_F64 ? 8.0 : 4.0;
        const double rows = (double)s->p->n / (double)c->world;
        const double iter_s = rows * (double)s->p->n * esz * (s->p->symmetric ? 0.5 : 1.0) / 5.0e12 + 30e-6;
        poll = (int64_t)(20.0e-3 / iter_s);
        poll = poll < 1 ? 1 : (poll > 64 ? 64 : poll);
    }
    // The product-bound solvers look at the flag with a LAG of one chunk: the copy of the flag is followed by an event,
    // the next chunk is enqueued at once, and only then does the host wait for that event — the device never runs dry
    // while the host decides (the extra chunk early-exits on the flag).  The factorising solvers enqueue O(n^3) work per
    // iteration from the host and check before every iteration.
    const bool lagged = poll > 0 && (s->kind == BQ_PG || s->kind == BQ_FW || s->kind == BQ_AL) && s->flag_host != nullptr;
    bool pending = false;
    for (int64_t k = 0; k < max_steps; ++k) {
        BQ_TRY(solver_iterate(s));
        if (s->kind == BQ_AS) {
            // ActiveSet looks at the device at the top of every iteration anyway (bq_as_iterate: the order of the restricted
            // system comes from there) and leaves s->host current: a second look here was one more stream drain per iteration
            if (s->host.done) break;
            continue;
        }
        if ((k + 1) % poll == 0 && k + 1 < max_steps) {
            if (lagged) {
                if (pending) {
                    BQ_TRY(bq_ctx_event_sync(c, s->flag_event));
                    if (*s->flag_host) break;
                }
                BQ_HIP(hipMemcpyAsync(s->flag_host, &s->sc->done, sizeof(int), hipMemcpyDeviceToHost, c->stream));
                BQ_HIP(hipEventRecord(s->flag_event, c->stream));
                pending = true;
            } else {
                BQ_HIP(hipMemcpyAsync(&s->host, s->sc, sizeof(bq_scal), hipMemcpyDeviceToHost, c->stream));
                BQ_SYNC(c);
                if (s->host.done) break;
            }
        }
    }
    if (s->al) BQ_TRY(bq_al_flush(s));
    BQ_HIP(hipMemcpyAsync(&s->host, s->sc, sizeof(bq_scal), hipMemcpyDeviceToHost, c->stream));
    BQ_SYNC(c);
    if (s->host.status < 0) {  // a kernel flagged a numerical failure (codes mirror BQ_ERR_*)
        bq_set_error(s->host.status == BQ_ERR_NOT_PD ? "Cholesky met a non-positive pivot"
                                                     : "non-finite values in the solver state");
        return s->host.status;
    }
    int64_t rows = s->host.iter - base + (s->host.done ? 1 : 0);
    if (rows > max_steps) rows = max_steps;
    if (rows < 0) rows = 0;
    if (stats && rows > 0) {
        BQ_HIP(hipMemcpyAsync(stats, s->stats, sizeof(bq_iter_stat) * rows, hipMemcpyDeviceToHost, c->stream));
        BQ_SYNC(c);
    }
    *n_stats = rows;
    *status = s->host.status;
    return BQ_OK;
}

extern "C" int bq_solver_state(const bq_solver *s, int64_t *iter, int *status, double *f_x) {
    BQ_ARG(s != nullptr, "solver is NULL");
    if (iter) *iter = s->host.iter;
    if (status) *status = s->host.status;
    if (f_x) *f_x = s->host.f;
    return BQ_OK;
}

extern "C" int bq_solver_get(bq_solver *s, int what, double *out) {
    BQ_ARG(s && out, "NULL argument");
    bq_ctx *c = s->p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    const double *src = nullptr;
    if (what == BQ_GET_DUAL) {
        BQ_ARG(s->al != nullptr, "multipliers exist for the augmented-Lagrangian solver only");
        const bq_al_vecs &V = s->al->V;
        double *o = out;
        if (V.a) *o++ = s->host.al_mu;
        for (const double *v : {(const double *)V.llb, (const double *)V.lub})
            if (v) {
                BQ_HIP(hipMemcpyAsync(o, v, sizeof(double) * s->N, hipMemcpyDeviceToHost, c->stream));
                o += s->N;
            }
        BQ_SYNC(c);
        return BQ_OK;
    }
    switch (what) {
        case BQ_GET_X: src = s->kind == BQ_AS ? bq_as_view(s, BQ_GET_X) : (s->al ? s->al->V.xe : s->x); break;
        case BQ_GET_G: src = s->kind == BQ_AS ? bq_as_view(s, BQ_GET_G) : s->g; break;
        case BQ_GET_X_NOW: src = s->x; break;
        case BQ_GET_G_NOW: src = s->g; break;
        case BQ_GET_D: src = s->d; break;
        case BQ_GET_LP: src = s->lp; break;
        case BQ_GET_LM: src = s->lm; break;
        default: break;
    }
    if (what == BQ_GET_MASK_L || what == BQ_GET_MASK_U) {
        const unsigned char *m = what == BQ_GET_MASK_L ? s->mL : s->mU;
        BQ_ARG(m != nullptr, "masks exist for ActiveSet only");
        std::vector<unsigned char> tmp((size_t)s->N);
        BQ_HIP(hipMemcpyAsync(tmp.data(), m, (size_t)s->N, hipMemcpyDeviceToHost, c->stream));
        BQ_SYNC(c);
        for (int64_t i = 0; i < s->N; ++i) out[i] = tmp[i] ? 1.0 : 0.0;
        return BQ_OK;
    }
    BQ_ARG(src != nullptr, "vector not available for this solver");
    BQ_HIP(hipMemcpyAsync(out, src, sizeof(double) * s->N, hipMemcpyDeviceToHost, c->stream));
    BQ_SYNC(c);
    return BQ_OK;
}

// ---- checkpoint / resume (bcqp.h) -----------------------------------------------------------------------------
// v + t dv with the device's rounding: one rounded product, one sum (pgfw_update_kernel / ip_update_kernel use __dmul_rn).
#pragma clang fp contract(off)
static void state_apply_step(std::vector<double> &v, const std::vector<double> &dv, double t) {
    for (size_t i = 0; i < v.size(); ++i) {
        const double prod = t * dv[i];
        v[i] = v[i] + prod;
    }
}

extern "C" int bq_solver_get_state(bq_solver *s, bq_solver_snapshot *out) {
    BQ_ARG(s && out, "NULL argument");
    BQ_ARG(s->kind != BQ_AL, "the augmented-Lagrangian solver keeps its state in x and BQ_GET_DUAL");
    bq_ctx *c = s->p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    const size_t N = (size_t)s->N;
    out->iter = s->host.iter;
    out->kind = s->as_cg ? BQ_AS_CG : s->kind;
    out->f = s->host.f;
    out->best_lb = s->host.best_lb;
    out->have = 0;
    // a decided step waits on the device until the next iteration's first kernel applies it — unless the run has ended
    // (the deciding kernels return before they form one) or has not begun
    const bool pending = s->started && !s->host.done && s->kind != BQ_AS;
    const double t = s->kind == BQ_IP ? s->host.step : s->host.t;
    std::vector<double> v(N), dv(N);
    auto down = [&](std::vector<double> &dst, const double *src) {
        return hipMemcpyAsync(dst.data(), src, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream);
    };
    auto fetch = [&](double *dst, const double *vec, const double *dvec) -> int {
        BQ_HIP(down(v, vec));
        if (pending) BQ_HIP(down(dv, dvec));
        BQ_SYNC(c);
        if (pending) state_apply_step(v, dv, t);
        memcpy(dst, v.data(), sizeof(double) * N);
        return BQ_OK;
    };
    const bool pgfw = s->kind == BQ_PG || s->kind == BQ_FW;
    if (out->x) {
        BQ_TRY(fetch(out->x, s->x, s->d));   // d: PG / FW direction, IP dx (ip_vecs)
        if (pgfw && pending) {   // bq_pgfw_compute keeps the stepped x in its box
            std::vector<double> lb(N), ub(N);
            BQ_HIP(down(lb, s->lb));
            BQ_HIP(down(ub, s->ub));
            BQ_SYNC(c);
            for (size_t i = 0; i < N; ++i) out->x[i] = out->x[i] < lb[i] ? lb[i] : (out->x[i] > ub[i] ? ub[i] : out->x[i]);
        }
        out->have |= BQ_STATE_X;
    }
    // the gradient exists once the start-up has run (PG / FW keep it current: g + t Qd; IP and ActiveSet keep the reference's
    // stale self.g_x: interior_point.py:180, active_set.py:157)
    if (out->g && s->initialised) {
        if (pgfw) {
            BQ_TRY(fetch(out->g, s->g, s->Qd));
        } else {
            BQ_HIP(down(v, s->g));
            BQ_SYNC(c);
            memcpy(out->g, v.data(), sizeof(double) * N);
        }
        out->have |= BQ_STATE_G;
    }
    if (s->kind == BQ_IP && out->lp && out->lm && s->initialised) {
        BQ_TRY(fetch(out->lp, s->lp, s->dlp));
        BQ_TRY(fetch(out->lm, s->lm, s->dlm));
        out->have |= BQ_STATE_MULT;
    }
    if (s->kind == BQ_AS && out->mask_l && out->mask_u && s->mL && s->mU) {
        BQ_TRY(bq_solver_get(s, BQ_GET_MASK_L, out->mask_l));
        BQ_TRY(bq_solver_get(s, BQ_GET_MASK_U, out->mask_u));
        out->have |= BQ_STATE_MASKS;
    }
    return BQ_OK;
}

extern "C" int bq_solver_set_state(bq_solver *s, const bq_solver_snapshot *in) {
    BQ_ARG(s && in, "NULL argument");
    BQ_ARG(s->kind != BQ_AL, "the augmented-Lagrangian solver is resumed through x0 / dual0 of bq_al_solver_create");
    BQ_ARG(!s->initialised, "the state can only be set before the solver's first run");
    BQ_ARG(in->kind == -1 || in->kind == (s->as_cg ? BQ_AS_CG : s->kind), "the state was taken from another kind of solver");
    BQ_ARG((in->have & BQ_STATE_X) && in->x, "a state holds x at least");
    BQ_ARG(in->iter >= 0, "iter must be >= 0");
    BQ_ARG(!(in->have & BQ_STATE_G) || in->g, "BQ_STATE_G without g");
    BQ_ARG(!(in->have & BQ_STATE_MULT) || (s->kind == BQ_IP && in->lp && in->lm), "BQ_STATE_MULT: lp and lm, InteriorPoint only");
    BQ_ARG(!(in->have & BQ_STATE_MASKS) || (s->kind == BQ_AS && in->mask_l && in->mask_u), "BQ_STATE_MASKS: mask_l and mask_u, ActiveSet only");
    bq_ctx *c = s->p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    const size_t N = (size_t)s->N;
    delete s->resume;
    s->resume = new bq_solver::resume_t();
    bq_solver::resume_t *r = s->resume;
    r->have = in->have & (BQ_STATE_G | BQ_STATE_MULT | BQ_STATE_MASKS);
    if (r->have & BQ_STATE_G) r->g.assign(in->g, in->g + N);
    if (r->have & BQ_STATE_MULT) {
        r->lp.assign(in->lp, in->lp + N);
        r->lm.assign(in->lm, in->lm + N);
    }
    if (r->have & BQ_STATE_MASKS) {
        r->mL.resize(N);
        r->mU.resize(N);
        for (size_t i = 0; i < N; ++i) {
            r->mL[i] = in->mask_l[i] != 0.0;
            r->mU[i] = in->mask_u[i] != 0.0;
            if (r->mL[i] && r->mU[i]) {
                bq_set_error("state: index %zu is in both masks (L and U are disjoint: active_set.py:85)", i);
                return BQ_ERR_BADARG;
            }
        }
    }
    s->host.iter = in->iter;
    if (s->kind == BQ_FW && in->best_lb == in->best_lb) s->host.best_lb = in->best_lb;
    BQ_HIP(hipMemcpyAsync(s->x, in->x, sizeof(double) * N, hipMemcpyHostToDevice, c->stream));
    BQ_HIP(hipMemcpyAsync(s->sc, &s->host, sizeof(bq_scal), hipMemcpyHostToDevice, c->stream));
    BQ_SYNC(c);
    return BQ_OK;
}
#pragma clang fp contract(on)
