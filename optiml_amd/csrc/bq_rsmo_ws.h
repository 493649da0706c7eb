// Working-set decomposition for the panel-free SMO (bq_rsmo_set_working_set, bcqp.h): the second stepping mode of bq_rsmo under
// BQ_RSMO_RULE_PLAIN.  Included by bq_rsmo.hip after its kernels; a solver on which bq_rsmo_set_working_set was never called launches
// nothing of this file.
//
// The two-variable step of bq_rsmo.hip reads the whole k-major image of X once or twice to change two variables.  Here an OUTER
// iteration picks a working set W of up to q <= WS_Q = 128 violators, solves the dual restricted to W on one compute unit, and
// applies the whole change of alpha to the gradient in ONE pass over the image, on the matrix cores:
//   ws_gather_kernel   (1 workgroup)   the rows v mod n of W from X into the k-major image Wt[dp][128] (zero beyond |W| and beyond d,
//                                      the padding of bq_gram_image.h), and a2, y, alpha, G and the boxes of W packed beside it
//   ws_kww_kernel      (1 workgroup)   K_WW = map(Wt Wt') by bq_mfma_tile_128 and rsmo_map, 128 x 128 fp64, to a 128 KB buffer
//   ws_local_kernel    (1 workgroup)   the sub-dual on W.  K_WW is copied into 128 KB of dynamic LDS (gfx950 has 160 KB per compute
//                                      unit; the Cholesky's diagonal kernel, bq_potrf_diag.hip, already lives on the same raised launch
//                                      attribute, so no global-memory variant is kept), then ONE wave iterates: lane l owns the slots
//                                      l and l + 64 in registers (alpha, g, y, box, diagonal), every pick is a butterfly of shuffles,
//                                      and there is no barrier in the loop.  An inner step is libsvm's: i = arg-max of -y g over
//                                      I_up, j by WSS2 from row i of K_WW (the diagonal taken from K_WW itself, so the 2 x 2 minors
//                                      are consistent; TAU guard), bq_rsmo_pair_update, g += the two scaled rows.  It stops when the
//                                      local gap is < max(tol, 0.1 x the gap at entry) (ThunderSVM's rule: late iterations do not
//                                      over-solve) or after 100 q updates; writes alpha_W and delta_s = y_s (alpha_s - old alpha_s).
//   ws_update_kernel   (mp / 128 workgroups)  THE HOT KERNEL.  Workgroup I forms the tile K[128 I .., W] by bq_mfma_tile_128 (image rows
//                                      from HBM, read exactly once per outer iteration; Wt is L2-resident), maps it in registers and
//                                      contracts every tile row with delta in a fixed order: a lane folds the 4 columns it holds
//                                      of each of its 16 rows, the 16 lanes that share a row meet through xor shuffles, the two
//                                      column waves through LDS.  G_v += y_v (K delta)_row(v) for the one or two variables of a row.
//                                      With the fresh G the workgroup sorts its candidates of each side — (-y G, v) over I_up and
//                                      (y G, v) over I_low — in LDS (bitonic network on the total order (value, larger index)) and
//                                      writes its best q of each side to a list of its own.
//   ws_merge_kernel    a tree over the lists, 16 per workgroup and level (n = 10^6: 7813 -> 489 -> 31 -> 2 -> 1 lists, four small
//                                      launches).  The last level is one workgroup that holds the q best of both sides: Gmax and
//                                      Gmax2 are the heads of the two lists, the stop test is libsvm's Gmax + Gmax2 < tol over ALL
//                                      variables, and the next W is the q / 2 best of I_up, then the best of I_low not yet taken
//                                      (a free variable is on both lists and is taken once), then, if I_low ran short, more of I_up.
//                                      The maximal violating pair is always in W, so libsvm's convergence argument carries over.
// No atomics, no order that depends on the grid or on timing: the same bits on every run and for every cut of bq_rsmo_run.
//
// K values come from MFMA tiles here: they do NOT have the bits of rsmo_row_value's fma chains, and a run takes other pairs than the
// two-variable mode.  This mode promises the same optimum within `tol` (the stop test is the same), not the same trajectory.
// The row cache is not used (bq_rsmo_rows still goes through it).
#pragma once

namespace {

constexpr int WS_Q = 128;                    // slots of a working set: columns of Wt, order of K_WW
constexpr int WS_FAN = 16;                   // lists per workgroup and level of the merge tree
constexpr int WS_SORT = WS_FAN * WS_Q;       // the longest sequence a merge sorts per side
constexpr size_t WS_LDS = sizeof(double) * WS_Q * WS_Q;
enum { WS_A2 = 0, WS_Y = 1, WS_ALPHA = 2, WS_G = 3, WS_BOX = 4, WS_PACK = 5 };   // the rows of rsmo_ws::pack

struct rsmo_ws {
    int q;                 // variables per working set
    int64_t dp;            // features of the image, padded
    int *W, *rowW;         // WS_Q: the variables of the working set (-1 beyond rsmo_ctl::wn) and their rows
    double *Wt;            // dp x WS_Q
    double *pack;          // WS_PACK x WS_Q
    double *Kww;           // WS_Q x WS_Q
    double *delta;         // WS_Q
    double *list_v;        // candidate lists, best first: entry r of side s (0: I_up, 1: I_low) of list L at (2 L + s) WS_Q + r
    int *list_i;           // ... its variable, -1: none
};

// every lane receives the winner of the wave under a total order (a butterfly: both lanes of a pair keep the same one)
template <typename ORDER>
__device__ __forceinline__ void ws_wave_pick(double &v, long long &idx, double &rider) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double v2 = __shfl_xor(v, off, 64);
        const long long i2 = __shfl_xor(idx, off, 64);
        const double k2 = __shfl_xor(rider, off, 64);
        if (ORDER::before(v2, i2, v, idx)) {
            v = v2;
            idx = i2;
            rider = k2;
        }
    }
}

// bitonic network over `sides` sequences of M (a power of two) entries each, laid end to end: every sequence best first under
// (value, larger index), entries without a variable (-1) last.  Called by the whole workgroup after a barrier; ends with one.
__device__ __forceinline__ void ws_bitonic(double *v, int *ix, int M, int sides) {
    for (int k = 2; k <= M; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int e = threadIdx.x; e < M * sides; e += RSMO_T) {
                const int p = e ^ j;
                if (p > e) {
                    const bool down = ((e & (M - 1)) & k) == 0;
                    const double va = v[e], vb = v[p];
                    const int ia = ix[e], ib = ix[p];
                    if (down ? bq_rsmo_max_before(vb, ib, va, ia) : bq_rsmo_max_before(va, ia, vb, ib)) {
                        v[e] = vb;
                        ix[e] = ib;
                        v[p] = va;
                        ix[p] = ia;
                    }
                }
            }
            __syncthreads();
        }
}

// The selection bq_rsmo_create_general made has resolved the row of its i into a cache slot that the two-variable mode's select kernel
// would fill.  This mode never launches that kernel: the resolve is undone, so that the cache is empty again and bq_rsmo_rows can
// never meet a slot that is assigned but was not written.  (A bq_rsmo_rows call before this one may have filled that very slot, hit_i
// says so, and other slots: those stay.  A freed slot has stamp 0, the first victim; the topmost one is handed out again in order.)
__global__ void ws_init_kernel(rsmo_dev P) {
    rsmo_ctl *c = P.ctl;
    const int slot = c->slot_i;
    if (slot >= 0 && !c->hit_i) {
        const int r = P.row_of[slot];
        if (r >= 0) P.slot_of[r] = -1;
        P.row_of[slot] = -1;
        P.stamp[slot] = 0;
        if (c->filled == slot + 1) c->filled = slot;
    }
    c->hits = 0;
    c->misses = 0;
    c->i = -1;
    c->slot_i = -1;
    c->hit_i = 0;
}

// ---- launch 1: the rows of W as an image, the scalars of W ------------------------------------------------------------------------
__global__ __launch_bounds__(RSMO_T) void ws_gather_kernel(rsmo_dev P, rsmo_ws S) {
    if (P.ctl->finished) return;
    __shared__ int row[WS_Q];
    const int tid = threadIdx.x;
    if (tid < WS_Q) {
        const int v = S.W[tid];
        const int r = (int)rsmo_row_of(P, v);
        row[tid] = r;
        S.rowW[tid] = r;
        S.pack[WS_A2 * WS_Q + tid] = v < 0 ? 0.0 : P.a2[r];
        S.pack[WS_Y * WS_Q + tid] = v < 0 ? 1.0 : P.y[v];
        S.pack[WS_ALPHA * WS_Q + tid] = v < 0 ? 0.0 : P.alpha[v];
        S.pack[WS_G * WS_Q + tid] = v < 0 ? 0.0 : P.G[v];
        S.pack[WS_BOX * WS_Q + tid] = v < 0 ? 0.0 : P.Cb[v];
    }
    __syncthreads();
    // consecutive threads read consecutive features of one row of X
    const int64_t total = S.dp * WS_Q;
    for (int64_t e = tid; e < total; e += RSMO_T) {
        const int s = (int)(e / S.dp);
        const int64_t k = e - (int64_t)s * S.dp;
        const int r = row[s];
        S.Wt[k * WS_Q + s] = r >= 0 && k < P.d ? P.X[(int64_t)r * P.d + k] : 0.0;
    }
}

// ---- launch 2: K_WW ----------------------------------------------------------------------------------------------------------------
template <int KIND, int DEG>
__global__ __launch_bounds__(RSMO_T) void ws_kww_kernel(rsmo_dev P, rsmo_ws S) {
    if (P.ctl->finished) return;
    __shared__ bq_tile_smem sm;
    bq_d4 acc[4][4];
    bq_tile_zero(acc);
    bq_mfma_tile_128(S.Wt, WS_Q, 0, S.Wt, WS_Q, 0, S.dp, sm, acc);
    const bool rbf = KIND == BQ_KERNEL_RBF;
    const double *a2 = S.pack + WS_A2 * WS_Q;
    bq_tile_foreach(acc, [&](int r, int c, double dot) {
        S.Kww[r * WS_Q + c] = rsmo_map<KIND, DEG>(P, dot, rbf ? a2[r] : 0.0, rbf ? a2[c] : 0.0, S.rowW[r] == S.rowW[c]);
    });
}

// ---- launch 3: the sub-dual on W, one wave on K_WW in LDS --------------------------------------------------------------------------
__global__ __launch_bounds__(RSMO_T) void ws_local_kernel(rsmo_dev P, rsmo_ws S) {
    rsmo_ctl *c = P.ctl;
    if (c->finished) return;
    extern __shared__ double ws_K[];
    for (int e = 2 * threadIdx.x; e < WS_Q * WS_Q; e += 2 * RSMO_T)
        *reinterpret_cast<bq_d2 *>(ws_K + e) = *reinterpret_cast<const bq_d2 *>(S.Kww + e);
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x, wn = c->wn;
    int v[2];
    double y[2], a[2], a0[2], g[2], box[2], kd[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int s = lane + 64 * h;
        v[h] = s < wn ? S.W[s] : -1;
        y[h] = S.pack[WS_Y * WS_Q + s];
        a[h] = a0[h] = S.pack[WS_ALPHA * WS_Q + s];
        g[h] = S.pack[WS_G * WS_Q + s];
        box[h] = S.pack[WS_BOX * WS_Q + s];
        kd[h] = ws_K[s * WS_Q + s];
    }
    auto at = [&](const double(&x)[2], int s) { return __shfl(s < 64 ? x[0] : x[1], s & 63, 64); };   // s is uniform
    const long long cap = 100LL * S.q;
    long long count = 0, last_i = -1, last_j = -1;
    double stop_at = 0.0;
    for (;;) {
        // i and the local gap
        double uv = -BQ_RSMO_INF, us = 0.0, low = -BQ_RSMO_INF;
        long long ui = -1;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (v[h] < 0) continue;
            if (bq_rsmo_in_up(y[h], a[h], box[h])) {
                const double val = bq_rsmo_up_value(y[h], g[h]);
                if (bq_rsmo_max_before(val, v[h], uv, ui)) {
                    uv = val;
                    ui = v[h];
                    us = (double)(lane + 64 * h);
                }
            }
            if (bq_rsmo_in_low(y[h], a[h], box[h])) low = fmax(low, bq_rsmo_low_value(y[h], g[h]));
        }
        ws_wave_pick<rsmo_max_order>(uv, ui, us);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) low = fmax(low, __shfl_xor(low, off, 64));
        if (ui < 0) break;
        const double gap = uv + low;
        if (count == 0) stop_at = fmax(P.tol, 0.1 * gap);
        if (gap < stop_at || count >= cap) break;
        const int si = (int)us;
        const double y_i = at(y, si), g_i = at(g, si), old_i = at(a, si), C_i = at(box, si), qd_i = at(kd, si);
        // j: WSS2 from row i of K_WW
        double bv = BQ_RSMO_INF, bs = 0.0, ki[2];
        long long bi = -1;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int s = lane + 64 * h;
            ki[h] = ws_K[si * WS_Q + s];
            if (v[h] < 0 || !bq_rsmo_in_low(y[h], a[h], box[h])) continue;
            bool ok;
            const double sc = bq_rsmo_score(uv, y[h], g[h], qd_i, kd[h], ki[h], &ok);
            if (ok && bq_rsmo_min_before(sc, v[h], bv, bi)) {
                bv = sc;
                bi = v[h];
                bs = (double)s;
            }
        }
        ws_wave_pick<rsmo_min_order>(bv, bi, bs);
        if (bi < 0) break;
        const int sj = (int)bs;
        const double y_j = at(y, sj), g_j = at(g, sj), old_j = at(a, sj), C_j = at(box, sj), qd_j = at(kd, sj);
        double a_i = old_i, a_j = old_j;
        bq_rsmo_pair_update(y_i, y_j, g_i, g_j, qd_i, qd_j, ws_K[si * WS_Q + sj], C_i, C_j, &a_i, &a_j);
        const double d_i = a_i - old_i, d_j = a_j - old_j;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int s = lane + 64 * h;
            if (s == si) a[h] = a_i;
            if (s == sj) a[h] = a_j;
            const double s_i = y_i * y[h], s_j = y_j * y[h];   // +-1: exact
            const double q_i = s_i * ki[h], q_j = s_j * ws_K[sj * WS_Q + s];
            g[h] = bq_rsmo_grad(g[h], q_i, d_i, q_j, d_j);
        }
        last_i = ui;
        last_j = bi;
        ++count;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const double moved = a[h] - a0[h];
        S.delta[lane + 64 * h] = v[h] < 0 ? 0.0 : y[h] * moved;
        if (v[h] >= 0) P.alpha[v[h]] = a[h];
    }
    if (lane == 0) {
        c->inner += count;
        if (count > 0) {
            c->last_i = (int)last_i;
            c->last_j = (int)last_j;
        }
    }
}

// ---- launch 4: G += y o (K[:, W] delta) in one pass over the image, then this workgroup's candidates ------------------------------
// first: the selection before the first outer iteration — no tile, no update, the candidates of the start gradient
template <int KIND, int DEG>
__global__ __launch_bounds__(RSMO_T) void ws_update_kernel(rsmo_dev P, rsmo_ws S, int first) {
    if (P.ctl->finished) return;
    __shared__ bq_tile_smem sm;
    __shared__ double red[2][BQ_GT];
    __shared__ double sv[2 * 2 * BQ_GT];
    __shared__ int si[2 * 2 * BQ_GT];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * BQ_GT;
    if (!first) {
        bq_d4 acc[4][4];
        bq_tile_zero(acc);
        bq_mfma_tile_128(P.At, P.mp, r0, S.Wt, WS_Q, 0, S.dp, sm, acc);
        const bool rbf = KIND == BQ_KERNEL_RBF;
        double dl[4], a2c[4];
        int rc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = bq_acc_col(j);
            dl[j] = S.delta[col];
            a2c[j] = rbf ? S.pack[WS_A2 * WS_Q + col] : 0.0;
            rc[j] = S.rowW[col];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = bq_acc_row(i, v);
                const int64_t t = r0 + row;
                const double a2t = rbf ? P.a2[t] : 0.0;
                double sum = 0.0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double k = rsmo_map<KIND, DEG>(P, acc[i][j][v], a2t, a2c[j], t == rc[j]);
                    const double term = k * dl[j];
                    sum = sum + term;
                }
#pragma unroll
                for (int off = 1; off < 16; off <<= 1) sum = sum + __shfl_xor(sum, off, 64);   // the 16 lanes that hold this row
                if ((tid & 15) == 0) red[(tid >> 6) & 1][row] = sum;
            }
        __syncthreads();
    }
    // thread -> variable: row r0 + (tid mod 128), the half tid / 128 of the 2n form
    const int64_t t = r0 + (tid & (BQ_GT - 1));
    const int64_t var = t + (int64_t)(tid >> 7) * P.n;
    double uval = -BQ_RSMO_INF, lval = -BQ_RSMO_INF;
    int ui = -1, li = -1;
    if (t < P.n && var < P.N) {
        const double y = P.y[var];
        double g = P.G[var];
        if (!first) {
            const double kd = red[0][tid & (BQ_GT - 1)] + red[1][tid & (BQ_GT - 1)];
            const double signed_kd = y * kd;
            g = g + signed_kd;
            P.G[var] = g;
        }
        const double a = P.alpha[var], C = P.Cb[var];
        if (bq_rsmo_in_up(y, a, C)) {
            uval = bq_rsmo_up_value(y, g);
            ui = (int)var;
        }
        if (bq_rsmo_in_low(y, a, C)) {
            lval = bq_rsmo_low_value(y, g);
            li = (int)var;
        }
    }
    sv[tid] = uval;
    si[tid] = ui;
    sv[2 * BQ_GT + tid] = lval;
    si[2 * BQ_GT + tid] = li;
    __syncthreads();
    ws_bitonic(sv, si, 2 * BQ_GT, 2);
    for (int e = tid; e < 2 * S.q; e += RSMO_T) {
        const int side = e / S.q, r = e - side * S.q;
        const int64_t at = ((int64_t)blockIdx.x * 2 + side) * WS_Q + r;
        S.list_v[at] = sv[side * 2 * BQ_GT + r];
        S.list_i[at] = si[side * 2 * BQ_GT + r];
    }
}

// ---- launch 5 (one per level): `count` lists from list `in` on, WS_FAN per workgroup; blockIdx.y the side -------------------------
// last: ONE workgroup takes both sides of the at most WS_FAN lists left, makes the next W and takes the scalar decisions
__global__ __launch_bounds__(RSMO_T) void ws_merge_kernel(rsmo_dev P, rsmo_ws S, int in, int count, int out, int last, int first) {
    rsmo_ctl *c = P.ctl;
    if (c->finished) return;
    __shared__ double sv[2 * WS_SORT];
    __shared__ int si[2 * WS_SORT];
    __shared__ int dup[2 * WS_Q];
    const int tid = threadIdx.x, q = S.q, sides = last ? 2 : 1;
    const int from = (int)blockIdx.x * WS_FAN, lists = count - from < WS_FAN ? count - from : WS_FAN;
    int M = 2;
    while (M < lists * q) M <<= 1;
    for (int e = tid; e < M * sides; e += RSMO_T) {
        const int side = last ? e / M : (int)blockIdx.y, pos = e & (M - 1);
        const int l = pos / q, r = pos - l * q;
        double val = -BQ_RSMO_INF;
        int idx = -1;
        if (l < lists) {
            const int64_t at = ((int64_t)(in + from + l) * 2 + side) * WS_Q + r;
            val = S.list_v[at];
            idx = S.list_i[at];
        }
        sv[e] = val;
        si[e] = idx;
    }
    __syncthreads();
    ws_bitonic(sv, si, M, sides);
    if (!last) {
        for (int r = tid; r < q; r += RSMO_T) {
            const int64_t at = ((int64_t)(out + blockIdx.x) * 2 + blockIdx.y) * WS_Q + r;
            S.list_v[at] = sv[r];
            S.list_i[at] = si[r];
        }
        return;
    }
    // U = si[0 .. q) the best of I_up, L = si[M .. M + q) the best of I_low.  dup[s]: L_s is among the q / 2 of U that W takes first;
    // dup[WS_Q + r]: U_r is on L
    const int half = q / 2;
    const int *U = si, *L = si + M;
    if (tid < WS_Q) {
        bool d = false;
        if (tid < q)
            for (int r = 0; r < half; ++r) d |= U[r] == L[tid];
        dup[tid] = d;
    } else {
        const int r = tid - WS_Q;
        bool d = false;
        if (r < q)
            for (int s = 0; s < q; ++s) d |= L[s] == U[r];
        dup[WS_Q + r] = d;
    }
    __syncthreads();
    if (tid != 0) return;
    int m = 0;
    for (int r = 0; r < half; ++r)
        if (U[r] >= 0) S.W[m++] = U[r];
    for (int s = 0; s < q && m < q; ++s)
        if (L[s] >= 0 && !dup[s]) S.W[m++] = L[s];
    for (int r = half; r < q && m < q; ++r)   // I_low ran short: I_up fills up
        if (U[r] >= 0 && !dup[WS_Q + r]) S.W[m++] = U[r];
    c->wn = m;
    for (; m < WS_Q; ++m) S.W[m] = -1;
    const double gmax = sv[0], gmax2 = sv[M];   // the heads of the lists: the maxima over ALL variables (-inf: an empty side)
    const long long steps = c->steps + (first ? 0 : 1);
    int fin = 0;
    if (U[0] < 0 || bq_rsmo_stop(gmax, gmax2, P.tol))
        fin = 1;
    else if (steps >= c->cap)
        fin = 2;
    c->steps = steps;
    c->gmax = gmax;
    c->gmax2 = gmax2;
    c->finished = fin;
}

}   // namespace
