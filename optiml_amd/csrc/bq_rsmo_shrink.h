// Shrinking for the panel-free SMO (bq_rsmo_set_shrinking, bcqp.h): libsvm's do_shrinking on a device-side active list, for the
// single-column solver under BQ_RSMO_RULE_PLAIN.  Included by bq_rsmo.hip after its kernels; a solver on which
// bq_rsmo_set_shrinking was never called launches nothing of this file.
//
// The active list.  An ascending list of the variables v in [0, N) that are still in the problem, in one of two buffers
// (rsmo_shr::act, rsmo_ctl::cur), its length in the control block (rsmo_ctl::nact); it starts as 0 .. N - 1.  The select, update
// and shrink kernels run over POSITIONS of the list: a thread of rsmo_lselect / rsmo_lupdate owns RSMO_LW = 4 consecutive
// positions (one 16-byte load of the list), a workgroup RSMO_T * RSMO_LW of them, and reads alpha, G, y, Cb, QD and the cached
// rows through v = act[p], t = v mod n.  The host sizes a grid by the last length it has read, an upper bound (the list only gets
// shorter between two reconstructions, and the host makes every reconstruction); workgroups past the list publish neutral
// partials and take the ticket.  All combines are the (value, larger index) orders of bq_rsmo_step.h, so a pick does not depend on
// the grid, and on the full list it is the pick of rsmo_select_kernel / rsmo_update_kernel bit for bit.
//
// Rows on the active set.  A miss computes K[r][t] at the columns t of active positions only, each value the ascending-feature
// fma chain of rsmo_row_value on x_r staged in LDS in chunks of RSMO_XCHUNK and the same rsmo_map: a value has the bits it has in
// a full row.  The four chains of a thread run interleaved.  Values go to the slot at their ORIGINAL column t; nothing is
// compacted in the cache.  In the 2n form the variables t and t + n may both be active: both positions compute the value and
// both write the same bits to row[t] (no deduplication).
//
// Cache validity.  A slot made on the active set A serves requests only while the active set is a subset of A.  Active sets are
// nested between two reconstructions, so one tag per slot is enough (rsmo_shr::slot_epoch): 0 = a full row, valid for ever;
// otherwise the epoch (rsmo_ctl::epoch, bumped by every reconstruction) in which the row was made.  A request that finds a slot of
// an earlier epoch is a miss that reuses the slot (rsmo_lresolve).  The tag is set when the slot is resolved, one launch before
// the row is made; a shrink pass may run in between (rsmo_lupdate's `shrink_next`), and the slot then takes the epoch's tag even
// while the list is still full.
//
// A shrink pass (rsmo_shrink_count_kernel, rsmo_shrink_scatter_kernel).  Gmax1 / Gmax2 are the maxima the update kernel has just
// reduced over the active set (rsmo_ctl::gmax, gmax2); bq_rsmo_be_shrunk is libsvm's be_shrunk.  The survivors are compacted in
// order: wave ballot and popcount, one count per workgroup, the ticket's last workgroup takes the exclusive prefix over the
// workgroups, the second launch scatters into the other buffer and its last workgroup flips the buffers.
//
// Control flow (svm.cpp: Solver::Solve, do_shrinking, reconstruct_gradient).  The host keeps libsvm's counter as the step number
// before which the next shrink pass runs and enqueues the pass there; the update launch before it is told (`shrink_next`).  What
// needs the full gradient stops the device: rsmo_ctl::pause, under which every launch returns at once like `finished`.
//   RSMO_PAUSE_UNSHRINK  the first shrink pass with Gmax1 + Gmax2 <= 10 tol on a shrunk list: the host reconstructs, makes everything
//                        active, runs the pass with the Gmax values taken before, and selects again;
//   RSMO_PAUSE_STOP      the stop test holds (or no partner exists) on a shrunk list: the host reconstructs, makes everything active
//                        and selects again — finished if it still holds, else on with a shrink pass after the next step.
// A stop test that holds right before a due shrink pass waits for it (rsmo_ctl::stop_pending), as in libsvm, where the pass comes
// first: on a shorter list the test still holds (both maxima can only fall), so the pass decides between finished and STOP.
//
// Requests.  hits + misses counts the row requests of steps, two per step, with one exception: a select that finds no partner on a
// shrunk list raises STOP after the update before it has requested (and counted) row i, and the selection after the reconstruction
// requests its i again; each such pause adds one request to which no step belongs.
#pragma once

namespace {

constexpr int RSMO_LW = 4;                       // list positions per thread
constexpr int RSMO_LTILE = RSMO_T * RSMO_LW;     // ... per workgroup
enum { RSMO_PAUSE_NONE = 0, RSMO_PAUSE_UNSHRINK = 1, RSMO_PAUSE_STOP = 2 };

struct rsmo_shr {
    int *act[2];         // the list's two buffers, N rounded up to RSMO_LW entries each
    int *slot_epoch;     // R: 0 a full row, else the epoch of the row in the slot
    double *lin;         // N: the linear term (G0 consumed it)
    int *flag;           // N: == stamp for the variables a reconstruction leaves alone
    int *wg_count, *wg_off;   // per workgroup of a shrink pass: survivors, and their exclusive prefix
};

// the positions of this thread: v[w] (0 when off), t[w] = v mod n, on[w]; live: the workgroup has a position on the list (uniform)
struct rsmo_lpos {
    int v[RSMO_LW], t[RSMO_LW];
    bool on[RSMO_LW], live;
};
__device__ __forceinline__ rsmo_lpos rsmo_positions(const rsmo_dev &P, const int *act, int nact) {
    rsmo_lpos q;
    q.live = (int64_t)blockIdx.x * RSMO_LTILE < nact;
    const int64_t p0 = ((int64_t)blockIdx.x * RSMO_T + threadIdx.x) * RSMO_LW;
    int4 four = make_int4(0, 0, 0, 0);
    if (p0 < nact) four = *reinterpret_cast<const int4 *>(act + p0);   // (the buffers are padded to a multiple of RSMO_LW)
    const int raw[RSMO_LW] = {four.x, four.y, four.z, four.w};
#pragma unroll
    for (int w = 0; w < RSMO_LW; ++w) {
        q.on[w] = p0 + w < nact;
        q.v[w] = q.on[w] ? raw[w] : 0;
        q.t[w] = q.v[w] >= P.n ? q.v[w] - (int)P.n : q.v[w];
    }
    return q;
}

// K[r][t[w]] for the positions of this thread (0 where off); called by every thread of the workgroup (barriers inside).  Each value
// is rsmo_row_value's chain; a position that is off runs its chain on column 0 and drops the result.  A workgroup past the end of
// the list (the host sizes the grid by the last length it read) has nothing to make and returns before the first barrier.
template <int KIND, int DEG>
__device__ __forceinline__ void rsmo_lrow_values(const rsmo_dev &P, int64_t r, const rsmo_lpos &q, double *xs, double (&kv)[RSMO_LW]) {
    double acc[RSMO_LW];
#pragma unroll
    for (int w = 0; w < RSMO_LW; ++w) acc[w] = kv[w] = 0.0;
    if (!q.live) return;
    for (int64_t k0 = 0; k0 < P.d; k0 += RSMO_XCHUNK) {
        const int len = (int)(P.d - k0 < RSMO_XCHUNK ? P.d - k0 : RSMO_XCHUNK);
        __syncthreads();
        for (int k = threadIdx.x; k < len; k += RSMO_T) xs[k] = P.X[r * P.d + k0 + k];
        __syncthreads();
        const double *col = P.At + k0 * P.mp;
#pragma unroll 4
        for (int k = 0; k < len; ++k) {
            const double x = xs[k];
            const double *at = col + (int64_t)k * P.mp;
#pragma unroll
            for (int w = 0; w < RSMO_LW; ++w) acc[w] = fma(x, at[q.t[w]], acc[w]);
        }
    }
    const bool rbf = KIND == BQ_KERNEL_RBF;
#pragma unroll
    for (int w = 0; w < RSMO_LW; ++w)
        kv[w] = q.on[w] ? rsmo_map<KIND, DEG>(P, acc[w], rbf ? P.a2[r] : 0.0, rbf ? P.a2[q.t[w]] : 0.0, q.t[w] == r) : 0.0;
}

// the row in `slot` at the positions of this thread: read on a hit, else made and written to the slot at its columns
template <int KIND, int DEG>
__device__ __forceinline__ void rsmo_lrow(const rsmo_dev &P, int64_t r, int slot, int hit, const rsmo_lpos &q, double *xs,
                                          double (&kv)[RSMO_LW]) {
    double *row = P.cache + (int64_t)slot * P.pitch;
    if (hit) {
#pragma unroll
        for (int w = 0; w < RSMO_LW; ++w) kv[w] = q.on[w] ? row[q.t[w]] : 0.0;
    } else {
        rsmo_lrow_values<KIND, DEG>(P, r, q, xs, kv);
#pragma unroll
        for (int w = 0; w < RSMO_LW; ++w)
            if (q.on[w]) row[q.t[w]] = kv[w];
    }
}

// rsmo_resolve with the slots' tags: a slot of an earlier epoch is a miss that keeps its slot; a miss takes `tag`.  whole: the
// caller reads every column of the row (bq_rsmo_rows), so a slot made on ANY shrunk list, this epoch's included, is such a miss.
// Called by every thread of the last workgroup; *hit is uniform.
__device__ __forceinline__ int rsmo_lresolve(const rsmo_dev &P, const rsmo_shr &S, int64_t r, int keep, int *hit,
                                             rsmo_pick_smem<long long> &sh, int tag, bool whole = false) {
    rsmo_ctl *c = P.ctl;
    const int have = P.slot_of[r];
    const int made = have >= 0 ? S.slot_epoch[have] : 0;
    if (made != 0 && (whole || made != c->epoch)) {
        __syncthreads();   // every thread has read the tables
        if (threadIdx.x == 0) {
            P.stamp[have] = ++c->clock;
            c->misses += 1;
            S.slot_epoch[have] = tag;
        }
        *hit = 0;
        __syncthreads();
        return have;
    }
    const int slot = rsmo_resolve(P, r, keep, hit, sh);
    if (!*hit && threadIdx.x == 0) S.slot_epoch[slot] = tag;
    __syncthreads();
    return slot;
}

// ---- launch 1 of a step on the list: rsmo_select_kernel<.., BQ_RSMO_RULE_PLAIN> over positions ---------------------------------------
template <int KIND, int DEG>
__global__ __launch_bounds__(RSMO_T) void rsmo_lselect_kernel(rsmo_dev P, rsmo_shr S) {
    rsmo_ctl *c = P.ctl;
    if (c->finished || c->pause || c->stop_pending) return;
    __shared__ double xs[RSMO_XCHUNK];
    __shared__ rsmo_pick_smem<double> sh;
    __shared__ rsmo_pick_smem<long long> shl;
    const int i = c->i, slot_i = c->slot_i, nact = c->nact, epoch = c->epoch;
    const double gmax = c->gmax;
    const int64_t r = rsmo_row_of(P, i);
    const rsmo_lpos q = rsmo_positions(P, S.act[c->cur], nact);
    double kv[RSMO_LW];
    rsmo_lrow<KIND, DEG>(P, r, slot_i, c->hit_i, q, xs, kv);
    const double qd_i = P.QD[r];
    double bv = BQ_RSMO_INF, bk = 0.0;
    long long bi = -1;
#pragma unroll
    for (int w = 0; w < RSMO_LW; ++w) {
        if (!q.on[w]) continue;
        const int v = q.v[w];
        const double y_t = P.y[v];
        if (!bq_rsmo_in_low(y_t, P.alpha[v], P.Cb[v])) continue;
        bool ok;
        const double sc = bq_rsmo_score(gmax, y_t, P.G[v], qd_i, P.QD[q.t[w]], kv[w], &ok);
        if (ok && bq_rsmo_min_before(sc, v, bv, bi)) {
            bv = sc;
            bi = v;
            bk = kv[w];
        }
    }
    rsmo_block_pick<rsmo_min_order>(bv, bi, bk, sh);
    if (threadIdx.x == 0) {
        bq_part_put(&P.part_v[blockIdx.x], bv);
        bq_part_put(&P.part_i[blockIdx.x], bi);
        bq_part_put(&P.part_k[blockIdx.x], bk);
    }
    if (!bq_last_block(&c->ticket, gridDim.x)) return;
    bv = BQ_RSMO_INF;
    bi = -1;
    bk = 0.0;
    for (unsigned int b = threadIdx.x; b < gridDim.x; b += RSMO_T) {
        const double v2 = bq_part_get(&P.part_v[b]);
        const long long i2 = bq_part_get(&P.part_i[b]);
        const double k2 = bq_part_get(&P.part_k[b]);
        if (bq_rsmo_min_before(v2, i2, bv, bi)) {
            bv = v2;
            bi = i2;
            bk = k2;
        }
    }
    rsmo_block_pick<rsmo_min_order>(bv, bi, bk, sh);
    if (bi < 0) {   // no partner (libsvm's Gmin_idx == -1): select_working_set returns 1
        if (threadIdx.x == 0) {
            if (nact < P.N)
                c->pause = RSMO_PAUSE_STOP;
            else
                c->finished = 1;
        }
        return;
    }
    const int j = (int)bi;
    const int64_t rj = j >= P.n ? j - P.n : j;
    int slot_j = slot_i, hit_j = 1;
    if (rj == r) {
        if (threadIdx.x == 0) rsmo_touch(P, slot_i);
    } else {
        slot_j = rsmo_lresolve(P, S, rj, slot_i, &hit_j, shl, nact < P.N ? epoch : 0);   // (the update launch makes it at once)
    }
    if (threadIdx.x == 0) {
        const double y_i = P.y[i], y_j = P.y[j];
        const double old_i = P.alpha[i], old_j = P.alpha[j];
        double a_i = old_i, a_j = old_j;
        bq_rsmo_pair_update(y_i, y_j, P.G[i], P.G[j], qd_i, P.QD[rj], bk, P.Cb[i], P.Cb[j], &a_i, &a_j);
        P.alpha[i] = a_i;
        P.alpha[j] = a_j;
        c->d_i = a_i - old_i;
        c->d_j = a_j - old_j;
        c->y_i = y_i;
        c->y_j = y_j;
        c->j = j;
        c->slot_j = slot_j;
        c->hit_j = hit_j;
        c->slot_u = slot_i;
        c->last_i = i;
        c->last_j = j;
    }
}

// ---- launch 2 of a step on the list: rsmo_update_kernel<.., BQ_RSMO_RULE_PLAIN> over positions; G moves at active variables only -------
// first: the selection alone (after a reconstruction).  shrink_next: a shrink pass follows this launch.
template <int KIND, int DEG>
__global__ __launch_bounds__(RSMO_T) void rsmo_lupdate_kernel(rsmo_dev P, rsmo_shr S, int first, int shrink_next) {
    rsmo_ctl *c = P.ctl;
    if (c->finished || c->pause || c->stop_pending) return;
    __shared__ double xs[RSMO_XCHUNK];
    __shared__ rsmo_pick_smem<double> sh;
    __shared__ rsmo_pick_smem<long long> shl;
    __shared__ double shw[RSMO_T / 64];
    const int nact = c->nact, epoch = c->epoch;
    const rsmo_lpos q = rsmo_positions(P, S.act[c->cur], nact);
    double g[RSMO_LW];
#pragma unroll
    for (int w = 0; w < RSMO_LW; ++w) g[w] = q.on[w] ? P.G[q.v[w]] : 0.0;
    if (!first) {
        const int j = c->j;
        const int64_t rj = j >= P.n ? j - P.n : j;
        const double d_i = c->d_i, d_j = c->d_j, y_i = c->y_i, y_j = c->y_j;
        const double *row_i = P.cache + (int64_t)c->slot_u * P.pitch;
        double kj[RSMO_LW];
        rsmo_lrow<KIND, DEG>(P, rj, c->slot_j, c->hit_j, q, xs, kj);
#pragma unroll
        for (int w = 0; w < RSMO_LW; ++w) {
            if (!q.on[w]) continue;
            const double y_t = P.y[q.v[w]];
            const double s_i = y_i * y_t, s_j = y_j * y_t;   // +-1: exact
            const double q_i = s_i * row_i[q.t[w]], q_j = s_j * kj[w];
            g[w] = bq_rsmo_grad(g[w], q_i, d_i, q_j, d_j);
            P.G[q.v[w]] = g[w];
        }
    }
    double uv = -BQ_RSMO_INF, rider = 0.0, low = -BQ_RSMO_INF;
    long long ui = -1;
#pragma unroll
    for (int w = 0; w < RSMO_LW; ++w) {
        if (!q.on[w]) continue;
        const int v = q.v[w];
        const double y_t = P.y[v], a = P.alpha[v], C = P.Cb[v];
        if (bq_rsmo_in_up(y_t, a, C)) {
            const double val = bq_rsmo_up_value(y_t, g[w]);
            if (bq_rsmo_max_before(val, v, uv, ui)) {
                uv = val;
                ui = v;
            }
        }
        if (bq_rsmo_in_low(y_t, a, C)) low = fmax(low, bq_rsmo_low_value(y_t, g[w]));
    }
    rsmo_block_pick<rsmo_max_order>(uv, ui, rider, sh);
    bq_wave_put<bq_op_max>(low, shw);
    __syncthreads();
    if (threadIdx.x == 0) {
        double w = shw[0];
        for (int k = 1; k < RSMO_T / 64; ++k) w = fmax(w, shw[k]);
        bq_part_put(&P.part_v[blockIdx.x], uv);
        bq_part_put(&P.part_i[blockIdx.x], ui);
        bq_part_put(&P.part_w[blockIdx.x], w);
    }
    if (!bq_last_block(&c->ticket, gridDim.x)) return;
    // what thread 0 rewrites at the end is read here, with barriers in between: every wave decides the tail below alike
    const long long steps = c->steps + (first ? 0 : 1);
    int unshrunk = c->unshrunk;
    uv = -BQ_RSMO_INF;
    ui = -1;
    low = -BQ_RSMO_INF;
    for (unsigned int b = threadIdx.x; b < gridDim.x; b += RSMO_T) {
        const double v2 = bq_part_get(&P.part_v[b]);
        const long long i2 = bq_part_get(&P.part_i[b]);
        if (bq_rsmo_max_before(v2, i2, uv, ui)) {
            uv = v2;
            ui = i2;
        }
        low = fmax(low, bq_part_get(&P.part_w[b]));
    }
    rsmo_block_pick<rsmo_max_order>(uv, ui, rider, sh);
    __syncthreads();
    bq_wave_put<bq_op_max>(low, shw);
    __syncthreads();
    low = shw[0];
    for (int k = 1; k < RSMO_T / 64; ++k) low = fmax(low, shw[k]);
    const bool stop = ui < 0 || bq_rsmo_stop(uv, low, P.tol);
    int fin = 0, pause = RSMO_PAUSE_NONE, pending = 0;
    if (!stop && steps >= c->cap) {
        fin = 2;   // (the host reconstructs before rho)
    } else {
        if (shrink_next && !unshrunk && bq_rsmo_unshrink(uv, low, P.tol)) {
            unshrunk = 1;
            if (nact < P.N) pause = RSMO_PAUSE_UNSHRINK;
        }
        if (stop && !pause) {
            if (shrink_next)
                pending = 1;
            else if (nact < P.N)
                pause = RSMO_PAUSE_STOP;
            else
                fin = 1;
        }
    }
    int slot = -1, hit = 0;
    if (!fin && !pause && !stop)
        slot = rsmo_lresolve(P, S, rsmo_row_of(P, (int)ui), -1, &hit, shl, nact < P.N || shrink_next ? epoch : 0);
    if (threadIdx.x == 0) {
        c->steps = steps;
        c->gmax = uv;
        c->gmax2 = low;
        c->i = (int)ui;
        c->slot_i = slot;
        c->hit_i = hit;
        c->finished = fin;
        c->pause = pause;
        c->stop_pending = pending;
        c->unshrunk = unshrunk;
    }
}

// ---- a shrink pass -----------------------------------------------------------------------------------------------------------------------
// does position p survive?  (p < nact, and libsvm's be_shrunk says no)
__device__ __forceinline__ bool rsmo_survives(const rsmo_dev &P, const int *act, int nact, int64_t p, double gmax, double gmax2, int *v) {
    if (p >= nact) return false;
    *v = act[p];
    return !bq_rsmo_be_shrunk(P.y[*v], P.alpha[*v], P.Cb[*v], P.G[*v], gmax, gmax2);
}

// launch 1: the survivors of each workgroup; the last workgroup takes the exclusive prefix over the workgroups and the new length
__global__ __launch_bounds__(RSMO_T) void rsmo_shrink_count_kernel(rsmo_dev P, rsmo_shr S) {
    rsmo_ctl *c = P.ctl;
    if (c->finished || c->pause) return;
    __shared__ int ws[RSMO_T / 64];
    const int nact = c->nact, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int v = 0;
    const bool keep = rsmo_survives(P, S.act[c->cur], nact, (int64_t)blockIdx.x * RSMO_T + threadIdx.x, c->gmax, c->gmax2, &v);
    const int cnt = __popcll(__ballot(keep));
    if (lane == 0) ws[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int k = 0; k < RSMO_T / 64; ++k) total += ws[k];
        bq_part_put(&S.wg_count[blockIdx.x], total);
    }
    if (!bq_last_block(&c->ticket, gridDim.x)) return;
    int carry = 0;
    for (unsigned int base = 0; base < gridDim.x; base += RSMO_T) {
        const unsigned int b = base + threadIdx.x;
        const int x = b < gridDim.x ? bq_part_get(&S.wg_count[b]) : 0;
        int incl = x;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        __syncthreads();   // ws is free (the first round: every thread has read its total; later rounds: the sums below)
        if (lane == 63) ws[wave] = incl;
        __syncthreads();
        int before = carry, all = 0;
        for (int k = 0; k < RSMO_T / 64; ++k) {
            if (k < wave) before += ws[k];
            all += ws[k];
        }
        if (b < gridDim.x) S.wg_off[b] = before + incl - x;
        carry += all;
    }
    if (threadIdx.x == 0) {
        c->nact_new = carry;
        c->scatter = 1;
        c->nshrink += 1;
        if (carry < c->min_act) c->min_act = carry;
        if (c->stop_pending) {   // the stop test held before this pass, and holds after it
            c->stop_pending = 0;
            if (carry < P.N)
                c->pause = RSMO_PAUSE_STOP;
            else
                c->finished = 1;
        }
    }
}

// launch 2: the survivors into the other buffer, in order; the last workgroup flips the buffers
__global__ __launch_bounds__(RSMO_T) void rsmo_shrink_scatter_kernel(rsmo_dev P, rsmo_shr S) {
    rsmo_ctl *c = P.ctl;
    if (!c->scatter) return;
    __shared__ int ws[RSMO_T / 64];
    const int nact = c->nact, cur = c->cur, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int v = 0;
    const bool keep = rsmo_survives(P, S.act[cur], nact, (int64_t)blockIdx.x * RSMO_T + threadIdx.x, c->gmax, c->gmax2, &v);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) ws[wave] = __popcll(mask);
    __syncthreads();
    if (keep) {
        int at = S.wg_off[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
        for (int k = 0; k < wave; ++k) at += ws[k];
        S.act[cur ^ 1][at] = v;   // at < nact_new <= N
    }
    if (!bq_last_block(&c->ticket, gridDim.x)) return;
    if (threadIdx.x == 0) {
        c->nact = c->nact_new;
        c->cur = cur ^ 1;
        c->scatter = 0;
    }
}

// ---- reconstruction ------------------------------------------------------------------------------------------------------------------------
// the list in hand marks its variables; everything else takes G_v = lin_v + s_v (K b)_row(v), rsmo_start_kernel's arithmetic
__global__ __launch_bounds__(RSMO_T) void rsmo_mark_kernel(rsmo_dev P, rsmo_shr S, int stamp) {
    const int64_t p = (int64_t)blockIdx.x * RSMO_T + threadIdx.x;
    if (p < P.ctl->nact) S.flag[S.act[P.ctl->cur][p]] = stamp;
}
__global__ __launch_bounds__(RSMO_T) void rsmo_rebuild_kernel(rsmo_dev P, rsmo_shr S, const double *Kb, int stamp) {
    const int64_t v = (int64_t)blockIdx.x * RSMO_T + threadIdx.x;
    if (v >= P.N || S.flag[v] == stamp) return;
    const double signed_kb = P.y[v] * Kb[v >= P.n ? v - P.n : v];
    P.G[v] = S.lin[v] + signed_kb;
}
// everything active again: the list 0 .. N - 1 in the buffer in hand, a new epoch, the pause lifted (first: the state of a new solver)
__global__ __launch_bounds__(RSMO_T) void rsmo_all_active_kernel(rsmo_dev P, rsmo_shr S, int first) {
    rsmo_ctl *c = P.ctl;
    const int64_t v = (int64_t)blockIdx.x * RSMO_T + threadIdx.x;
    if (v < P.N) S.act[first ? 0 : c->cur][v] = (int)v;
    if (v == 0) {   // (no thread of this launch reads what is written here)
        c->nact = (int)P.N;
        c->epoch += 1;
        c->pause = RSMO_PAUSE_NONE;
        c->stop_pending = 0;
        if (first) c->min_act = (int)P.N;
    }
}

// ---- bq_rsmo_rows on a solver with shrinking: rsmo_request_kernel with the slots' tags -------------------------------------------------------
// rsmo_fill_kernel copies all n columns of a hit, so only a full row (tag 0) is one: a slot made on a shrunk list, of whatever epoch,
// is a miss that the fill makes whole in place (tag 0 from then on; the values a step has read from it keep their bits).
__global__ __launch_bounds__(RSMO_T) void rsmo_lrequest_kernel(rsmo_dev P, rsmo_shr S, int64_t r) {
    __shared__ rsmo_pick_smem<long long> shl;
    rsmo_ctl *c = P.ctl;
    const int pending = c->finished ? -1 : c->slot_i, computed = c->hit_i;
    int hit = 0;
    const int slot = rsmo_lresolve(P, S, r, pending, &hit, shl, 0, true);
    if (threadIdx.x == 0) {
        if (slot == pending && !computed) {   // the pending row's slot, not yet filled: the request fills it, whole
            hit = 0;
            c->hit_i = 1;
            S.slot_epoch[slot] = 0;
        }
        c->req_slot = slot;
        c->req_hit = hit;
    }
}

}   // namespace
