// The batched panel-free SMO under BQ_RSMO_RULE_NU (libsvm's Solver_NU, the scalar rules of bq_rsmo_step.h) and the start gradient
// of nonzero starts — included by bq_mrsmo.hip after its own kernels, whose structures, tables and memory discipline these share.
//
// A Solver_NU step of all live columns is the same four launches.  Launch 4 (update) picks ONE maximal violator per sign (ip over
// y = +1, in over y = -1) and asks for both rows: two requests per column, -1 for a side without a violator, resolved together by
// mr_resolve_last<2> (ip and in on one row — nu-SVR's t and t + n — share a slot, the second request a hit).  Launch 2 (select)
// scores every variable against the row of ITS OWN sign, so a position reads one of the column's two cached rows, chosen per lane;
// j and with it i = ip or in, the pair update, and the request for row j with both i-rows pinned.  Launch 4 of the next step reads
// the row of the i that was paired (slot_u) and the row of j.
//
// The start.  G0_v = lin_v + s_v acc_v, acc_v the sum over the rows r of the column with b_r != 0 (b folded to the rows, or per
// position of a list), ascending, of fl(K[row(v)][r] b_r): one rounded product and one rounded add per row, so NumPy restates it.
// The host walks the ascending union of those rows over all columns in batches that fit the cache; a batch goes through
// mr_request_kernel / mr_rows_kernel (16 rows per MFMA pass, made ONCE for every column that has it) and one start kernel folds it
// into every column: K[row(v)][r] = K[r][row(v)] bit for bit, so a thread reads the cached row r at its own column(s) — coalesced
// in the full form, through the list in the list form — and keeps its accumulators in registers across the batch.
#pragma once

namespace {

__device__ __forceinline__ int mr_row_of(const mr_dev &P, long long v) { return v < 0 ? -1 : (int)(v >= P.n ? v - P.n : v); }

// what thread 0 of a column's last workgroup does once j is known: i = ip or in by the sign of j, the pair update, the j request;
// no partner (libsvm's Gmin_idx == -1): the column is finished and asks for nothing in either phase
__device__ __forceinline__ void mr_nu_pair(const mr_dev &P, int c, mr_col *cc, double *al, const double *G, const double *y, const double *Cb,
                                           long long bi, double bk, double qd_p, double qd_n, double qd_j, int rj) {
    if (bi < 0) {
        cc->finished = 1;
        bq_part_put(&P.req_row[c], -1);
        bq_part_put(&P.req_row[P.k + 2 * c], -1);
        bq_part_put(&P.req_row[P.k + 2 * c + 1], -1);
        return;
    }
    const int j = (int)bi;
    const bool neg = y[j] < 0.0;
    const int iu = neg ? cc->i2 : cc->i;
    const double y_i = y[iu], y_j = y[j];
    const double old_i = al[iu], old_j = al[j];
    double a_i = old_i, a_j = old_j;
    bq_rsmo_pair_update(y_i, y_j, G[iu], G[j], neg ? qd_n : qd_p, qd_j, bk, Cb[iu], Cb[j], &a_i, &a_j);
    al[iu] = a_i;
    al[j] = a_j;
    cc->d_i = a_i - old_i;
    cc->d_j = a_j - old_j;
    cc->y_i = y_i;
    cc->y_j = y_j;
    cc->j = j;
    cc->slot_u = neg ? cc->slot_2 : cc->slot_i;
    cc->last_i = iu;
    cc->last_j = j;
    bq_part_put(&P.req_row[c], rj);
}

// what thread 0 of a column's last workgroup does with the two arg-maxima and the two I_low maxima: the stop test, the next (ip, in)
// and their two requests (rp / rn: the rows of ui / ni, -1 without one)
__device__ __forceinline__ void mr_nu_next(const mr_dev &P, int c, mr_col *cc, int first, double uv, long long ui, double low, double nv,
                                           long long ni, double lown, int rp, int rn) {
    const long long steps = cc->steps + (first ? 0 : 1);
    int fin = 0;
    if ((ui < 0 && ni < 0) || bq_rsmo_nu_stop(uv, low, nv, lown, P.tol))
        fin = 1;
    else if (steps >= P.glob->cap)
        fin = 2;
    cc->steps = steps;
    cc->gmax = uv;
    cc->gmax2 = low;
    cc->gmaxn = nv;
    cc->gmaxn2 = lown;
    cc->i = (int)ui;
    cc->i2 = (int)ni;
    cc->finished = fin;
    bq_part_put(&P.req_row[P.k + 2 * c], fin ? -1 : rp);
    bq_part_put(&P.req_row[P.k + 2 * c + 1], fin ? -1 : rn);
    if (fin) bq_part_put(&P.req_row[c], -1);
}

// the maximum of the waves' I_low maxima (bq_wave_put), by thread 0 after a barrier
__device__ __forceinline__ double mr_waves_max(const double *shw) {
    double w = shw[0];
    for (int q = 1; q < RSMO_T / 64; ++q) w = fmax(w, shw[q]);
    return w;
}

// ---- launch 2, full columns -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RSMO_T) void mr_nu_select_kernel(mr_dev P) {
    const int c = blockIdx.y;
    mr_col *cc = &P.col[c];
    const int live = P.glob->live;
    if (cc->finished) return;
    __shared__ rsmo_pick_smem<double> sh;
    __shared__ rsmo_pick_smem<long long> shl;
    const double *alpha = P.alpha + (int64_t)c * P.N, *G = P.G + (int64_t)c * P.N, *y = P.y + (int64_t)c * P.N,
                 *Cb = P.Cb + (int64_t)c * P.N;
    const int ip = cc->i, in = cc->i2;
    const double gmaxp = cc->gmax, gmaxn = cc->gmaxn;
    const double *row_p = P.cache + (int64_t)(cc->slot_i < 0 ? 0 : cc->slot_i) * P.pitch;
    const double *row_n = P.cache + (int64_t)(cc->slot_2 < 0 ? 0 : cc->slot_2) * P.pitch;
    const double qd_p = ip >= 0 ? P.QD[mr_row_of(P, ip)] : 0.0, qd_n = in >= 0 ? P.QD[mr_row_of(P, in)] : 0.0;
    const int64_t t = (int64_t)blockIdx.x * RSMO_T + threadIdx.x;
    double bv = BQ_RSMO_INF, bk = 0.0;
    long long bi = -1;
    if (t < P.n) {
        const double qd_t = P.QD[t];
        for (int64_t v = t; v < P.N; v += P.n) {   // 2n variables: t (+1) and t + n (-1) share the row index, not the row read
            const double y_t = y[v];
            const bool neg = y_t < 0.0;
            if ((neg ? in : ip) < 0 || !bq_rsmo_in_low(y_t, alpha[v], Cb[v])) continue;   // (no violator of this sign: Gmax = -inf)
            const double k = (neg ? row_n : row_p)[t];
            bool ok;
            const double sc = bq_rsmo_nu_score(y_t, G[v], gmaxp, qd_p, k, gmaxn, qd_n, k, qd_t, &ok);
            if (ok && bq_rsmo_min_before(sc, v, bv, bi)) {
                bv = sc;
                bi = v;
                bk = k;
            }
        }
    }
    rsmo_block_pick<rsmo_min_order>(bv, bi, bk, sh);
    const int64_t pb = (int64_t)c * gridDim.x;
    if (threadIdx.x == 0) {
        bq_part_put(&P.part_v[pb + blockIdx.x], bv);
        bq_part_put(&P.part_i[pb + blockIdx.x], bi);
        bq_part_put(&P.part_k[pb + blockIdx.x], bk);
    }
    if (!bq_last_block(&cc->ticket, gridDim.x)) return;
    bv = BQ_RSMO_INF;
    bi = -1;
    bk = 0.0;
    for (unsigned int b = threadIdx.x; b < gridDim.x; b += RSMO_T) {
        const double v2 = bq_part_get(&P.part_v[pb + b]);
        const long long i2 = bq_part_get(&P.part_i[pb + b]);
        const double k2 = bq_part_get(&P.part_k[pb + b]);
        if (bq_rsmo_min_before(v2, i2, bv, bi)) {
            bv = v2;
            bi = i2;
            bk = k2;
        }
    }
    rsmo_block_pick<rsmo_min_order>(bv, bi, bk, sh);
    if (threadIdx.x == 0) {
        const int rj = mr_row_of(P, bi);
        mr_nu_pair(P, c, cc, P.alpha + (int64_t)c * P.N, G, y, Cb, bi, bk, qd_p, qd_n, rj >= 0 ? P.QD[rj] : 0.0, rj);
    }
    if (!bq_last_block(&P.glob->ticket, (unsigned int)live)) return;
    mr_resolve_last<2>(P, shl, true);
}

// ---- launch 4, full columns -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RSMO_T) void mr_nu_update_kernel(mr_dev P, int first) {
    const int c = blockIdx.y;
    mr_col *cc = &P.col[c];
    const int live = P.glob->live;
    if (cc->finished) return;
    __shared__ rsmo_pick_smem<double> sh;
    __shared__ rsmo_pick_smem<long long> shl;
    __shared__ double shw[RSMO_T / 64], shw2[RSMO_T / 64];
    const double *alpha = P.alpha + (int64_t)c * P.N, *y = P.y + (int64_t)c * P.N, *Cb = P.Cb + (int64_t)c * P.N;
    double *G = P.G + (int64_t)c * P.N;
    const int64_t t = (int64_t)blockIdx.x * RSMO_T + threadIdx.x;
    double g[2] = {0.0, 0.0};
    if (t < P.n) {
        g[0] = G[t];
        if (P.N > P.n) g[1] = G[t + P.n];
    }
    if (!first && t < P.n) {
        const double d_i = cc->d_i, d_j = cc->d_j, y_i = cc->y_i, y_j = cc->y_j;
        const double ki = P.cache[(int64_t)(cc->slot_u < 0 ? 0 : cc->slot_u) * P.pitch + t];
        const double kj = P.cache[(int64_t)(cc->slot_j < 0 ? 0 : cc->slot_j) * P.pitch + t];
        int h = 0;
        for (int64_t v = t; v < P.N; v += P.n, ++h) {
            const double y_t = y[v];
            const double s_i = y_i * y_t, s_j = y_j * y_t;   // +-1: exact
            const double q_i = s_i * ki, q_j = s_j * kj;
            g[h] = bq_rsmo_grad(g[h], q_i, d_i, q_j, d_j);
            G[v] = g[h];
        }
    }
    // (uv, ui) / low: the arg-max over I_up and the maximum over I_low of the positive sign, (nv, ni) / lown of the negative
    double uv = -BQ_RSMO_INF, rider = 0.0, low = -BQ_RSMO_INF, nv = -BQ_RSMO_INF, lown = -BQ_RSMO_INF;
    long long ui = -1, ni = -1;
    if (t < P.n) {
        int h = 0;
        for (int64_t v = t; v < P.N; v += P.n, ++h) {
            const double y_t = y[v], a = alpha[v], C = Cb[v];
            const bool neg = y_t < 0.0;
            if (bq_rsmo_in_up(y_t, a, C)) {
                const double val = bq_rsmo_up_value(y_t, g[h]);
                if (neg) {
                    if (bq_rsmo_max_before(val, v, nv, ni)) {
                        nv = val;
                        ni = v;
                    }
                } else if (bq_rsmo_max_before(val, v, uv, ui)) {
                    uv = val;
                    ui = v;
                }
            }
            if (bq_rsmo_in_low(y_t, a, C)) {
                const double val = bq_rsmo_low_value(y_t, g[h]);
                if (neg)
                    lown = fmax(lown, val);
                else
                    low = fmax(low, val);
            }
        }
    }
    rsmo_block_pick<rsmo_max_order>(uv, ui, rider, sh);
    rsmo_block_pick<rsmo_max_order>(nv, ni, rider, sh);
    bq_wave_put<bq_op_max>(low, shw);
    bq_wave_put<bq_op_max>(lown, shw2);
    __syncthreads();
    const int64_t pb = (int64_t)c * gridDim.x;
    if (threadIdx.x == 0) {
        bq_part_put(&P.part_v[pb + blockIdx.x], uv);
        bq_part_put(&P.part_i[pb + blockIdx.x], ui);
        bq_part_put(&P.part_w[pb + blockIdx.x], mr_waves_max(shw));
        bq_part_put(&P.part_v2[pb + blockIdx.x], nv);
        bq_part_put(&P.part_i2[pb + blockIdx.x], ni);
        bq_part_put(&P.part_w2[pb + blockIdx.x], mr_waves_max(shw2));
    }
    if (!bq_last_block(&cc->ticket, gridDim.x)) return;
    uv = nv = low = lown = -BQ_RSMO_INF;
    ui = ni = -1;
    for (unsigned int b = threadIdx.x; b < gridDim.x; b += RSMO_T) {
        const double v2 = bq_part_get(&P.part_v[pb + b]), v3 = bq_part_get(&P.part_v2[pb + b]);
        const long long i2 = bq_part_get(&P.part_i[pb + b]), i3 = bq_part_get(&P.part_i2[pb + b]);
        if (bq_rsmo_max_before(v2, i2, uv, ui)) {
            uv = v2;
            ui = i2;
        }
        if (bq_rsmo_max_before(v3, i3, nv, ni)) {
            nv = v3;
            ni = i3;
        }
        low = fmax(low, bq_part_get(&P.part_w[pb + b]));
        lown = fmax(lown, bq_part_get(&P.part_w2[pb + b]));
    }
    rsmo_block_pick<rsmo_max_order>(uv, ui, rider, sh);
    rsmo_block_pick<rsmo_max_order>(nv, ni, rider, sh);
    __syncthreads();
    bq_wave_put<bq_op_max>(low, shw);
    bq_wave_put<bq_op_max>(lown, shw2);
    __syncthreads();
    if (threadIdx.x == 0)
        mr_nu_next(P, c, cc, first, uv, ui, mr_waves_max(shw), nv, ni, mr_waves_max(shw2), mr_row_of(P, ui), mr_row_of(P, ni));
    if (!bq_last_block(&P.glob->ticket, (unsigned int)live)) return;
    mr_resolve_last<2>(P, shl, false);
}

// ---- launch 2, row lists --------------------------------------------------------------------------------------------------------------
template <int PER>
__global__ __launch_bounds__(RSMO_T) void ml_nu_select_kernel(mr_dev P) {
    const int2 wk = P.work[blockIdx.x];
    const int c = wk.x;
    mr_col *cc = &P.col[c];
    const int live = P.glob->live;
    if (cc->finished) return;
    __shared__ rsmo_pick_smem<double> sh;
    __shared__ rsmo_pick_smem<long long> shl;
    const ml_info in = P.info[c];
    const double *alpha = P.alpha + in.off, *G = P.G + in.off, *y = P.y + in.off, *Cb = P.Cb + in.off;
    const int *rows = P.rows + in.off;
    const int ip = cc->i, i_n = cc->i2;
    const double gmaxp = cc->gmax, gmaxn = cc->gmaxn;
    const double *row_p = P.cache + (int64_t)(cc->slot_i < 0 ? 0 : cc->slot_i) * P.pitch;
    const double *row_n = P.cache + (int64_t)(cc->slot_2 < 0 ? 0 : cc->slot_2) * P.pitch;
    const double qd_p = ip >= 0 ? P.QD[rows[ip]] : 0.0, qd_n = i_n >= 0 ? P.QD[rows[i_n]] : 0.0;
    const int q0 = wk.y + PER * (int)threadIdx.x;
    double bv = BQ_RSMO_INF, bk = 0.0;
    long long bi = -1;
    if (q0 < in.m) {   // q0 + PER - 1 lies inside the column's padded length: the pad positions hold a valid row and are not scanned
        double a_t[PER], g_t[PER], y_t[PER], C_t[PER], k_t[PER], qd_t[PER];
        int r_t[PER];
        ml_load<PER>(rows + q0, r_t);
        ml_load<PER>(y + q0, y_t);
        ml_load<PER>(alpha + q0, a_t);
        ml_load<PER>(Cb + q0, C_t);
        ml_load<PER>(G + q0, g_t);
#pragma unroll
        for (int e = 0; e < PER; ++e) {   // the gathers go out together: each position from the row of its own sign
            k_t[e] = (y_t[e] < 0.0 ? row_n : row_p)[r_t[e]];
            qd_t[e] = P.QD[r_t[e]];
        }
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            if (q0 + e >= in.m || (y_t[e] < 0.0 ? i_n : ip) < 0 || !bq_rsmo_in_low(y_t[e], a_t[e], C_t[e])) continue;
            bool ok;
            const double sc = bq_rsmo_nu_score(y_t[e], g_t[e], gmaxp, qd_p, k_t[e], gmaxn, qd_n, k_t[e], qd_t[e], &ok);
            if (ok && bq_rsmo_min_before(sc, q0 + e, bv, bi)) {
                bv = sc;
                bi = q0 + e;
                bk = k_t[e];
            }
        }
    }
    rsmo_block_pick<rsmo_min_order>(bv, bi, bk, sh);
    const int64_t pb = in.part0, mine = pb + wk.y / (RSMO_T * PER);
    if (threadIdx.x == 0) {
        bq_part_put(&P.part_v[mine], bv);
        bq_part_put(&P.part_i[mine], bi);
        bq_part_put(&P.part_k[mine], bk);
    }
    if (!bq_last_block(&cc->ticket, (unsigned int)in.nsl)) return;
    bv = BQ_RSMO_INF;
    bi = -1;
    bk = 0.0;
    for (int b = threadIdx.x; b < in.nsl; b += RSMO_T) {
        const double v2 = bq_part_get(&P.part_v[pb + b]);
        const long long i2 = bq_part_get(&P.part_i[pb + b]);
        const double k2 = bq_part_get(&P.part_k[pb + b]);
        if (bq_rsmo_min_before(v2, i2, bv, bi)) {
            bv = v2;
            bi = i2;
            bk = k2;
        }
    }
    rsmo_block_pick<rsmo_min_order>(bv, bi, bk, sh);
    if (threadIdx.x == 0) {
        const int rj = bi < 0 ? -1 : rows[bi];
        mr_nu_pair(P, c, cc, P.alpha + in.off, G, y, Cb, bi, bk, qd_p, qd_n, rj >= 0 ? P.QD[rj] : 0.0, rj);
    }
    if (!bq_last_block(&P.glob->ticket, (unsigned int)live)) return;
    mr_resolve_last<2>(P, shl, true);
}

// ---- launch 4, row lists --------------------------------------------------------------------------------------------------------------
template <int PER>
__global__ __launch_bounds__(RSMO_T) void ml_nu_update_kernel(mr_dev P, int first) {
    const int2 wk = P.work[blockIdx.x];
    const int c = wk.x;
    mr_col *cc = &P.col[c];
    const int live = P.glob->live;
    if (cc->finished) return;
    __shared__ rsmo_pick_smem<double> sh;
    __shared__ rsmo_pick_smem<long long> shl;
    __shared__ double shw[RSMO_T / 64], shw2[RSMO_T / 64];
    const ml_info in = P.info[c];
    const double *alpha = P.alpha + in.off, *y = P.y + in.off, *Cb = P.Cb + in.off;
    double *G = P.G + in.off;
    const int *rows = P.rows + in.off;
    const int q0 = wk.y + PER * (int)threadIdx.x;
    double uv = -BQ_RSMO_INF, rider = 0.0, low = -BQ_RSMO_INF, nv = -BQ_RSMO_INF, lown = -BQ_RSMO_INF;
    long long ui = -1, ni = -1;
    if (q0 < in.m) {
        double a_t[PER], g_t[PER], y_t[PER], C_t[PER];
        ml_load<PER>(y + q0, y_t);
        ml_load<PER>(G + q0, g_t);
        if (!first) {
            int r_t[PER];
            double ki[PER], kj[PER];
            ml_load<PER>(rows + q0, r_t);
            const double d_i = cc->d_i, d_j = cc->d_j, y_i = cc->y_i, y_j = cc->y_j;
            const double *row_i = P.cache + (int64_t)(cc->slot_u < 0 ? 0 : cc->slot_u) * P.pitch;
            const double *row_j = P.cache + (int64_t)(cc->slot_j < 0 ? 0 : cc->slot_j) * P.pitch;
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                ki[e] = row_i[r_t[e]];
                kj[e] = row_j[r_t[e]];
            }
#pragma unroll
            for (int e = 0; e < PER; ++e) {   // (a pad position follows its column's last row; nobody reads it)
                const double s_i = y_i * y_t[e], s_j = y_j * y_t[e];   // +-1: exact
                const double q_i = s_i * ki[e], q_j = s_j * kj[e];
                g_t[e] = bq_rsmo_grad(g_t[e], q_i, d_i, q_j, d_j);
            }
#pragma unroll
            for (int u = 0; u < PER / 2; ++u) reinterpret_cast<bq_d2 *>(G + q0)[u] = (bq_d2){g_t[2 * u], g_t[2 * u + 1]};
        }
        ml_load<PER>(alpha + q0, a_t);
        ml_load<PER>(Cb + q0, C_t);
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            if (q0 + e >= in.m) continue;
            const bool neg = y_t[e] < 0.0;
            if (bq_rsmo_in_up(y_t[e], a_t[e], C_t[e])) {
                const double val = bq_rsmo_up_value(y_t[e], g_t[e]);
                if (neg) {
                    if (bq_rsmo_max_before(val, q0 + e, nv, ni)) {
                        nv = val;
                        ni = q0 + e;
                    }
                } else if (bq_rsmo_max_before(val, q0 + e, uv, ui)) {
                    uv = val;
                    ui = q0 + e;
                }
            }
            if (bq_rsmo_in_low(y_t[e], a_t[e], C_t[e])) {
                const double val = bq_rsmo_low_value(y_t[e], g_t[e]);
                if (neg)
                    lown = fmax(lown, val);
                else
                    low = fmax(low, val);
            }
        }
    }
    rsmo_block_pick<rsmo_max_order>(uv, ui, rider, sh);
    rsmo_block_pick<rsmo_max_order>(nv, ni, rider, sh);
    bq_wave_put<bq_op_max>(low, shw);
    bq_wave_put<bq_op_max>(lown, shw2);
    __syncthreads();
    const int64_t pb = in.part0, mine = pb + wk.y / (RSMO_T * PER);
    if (threadIdx.x == 0) {
        bq_part_put(&P.part_v[mine], uv);
        bq_part_put(&P.part_i[mine], ui);
        bq_part_put(&P.part_w[mine], mr_waves_max(shw));
        bq_part_put(&P.part_v2[mine], nv);
        bq_part_put(&P.part_i2[mine], ni);
        bq_part_put(&P.part_w2[mine], mr_waves_max(shw2));
    }
    if (!bq_last_block(&cc->ticket, (unsigned int)in.nsl)) return;
    uv = nv = low = lown = -BQ_RSMO_INF;
    ui = ni = -1;
    for (int b = threadIdx.x; b < in.nsl; b += RSMO_T) {
        const double v2 = bq_part_get(&P.part_v[pb + b]), v3 = bq_part_get(&P.part_v2[pb + b]);
        const long long i2 = bq_part_get(&P.part_i[pb + b]), i3 = bq_part_get(&P.part_i2[pb + b]);
        if (bq_rsmo_max_before(v2, i2, uv, ui)) {
            uv = v2;
            ui = i2;
        }
        if (bq_rsmo_max_before(v3, i3, nv, ni)) {
            nv = v3;
            ni = i3;
        }
        low = fmax(low, bq_part_get(&P.part_w[pb + b]));
        lown = fmax(lown, bq_part_get(&P.part_w2[pb + b]));
    }
    rsmo_block_pick<rsmo_max_order>(uv, ui, rider, sh);
    rsmo_block_pick<rsmo_max_order>(nv, ni, rider, sh);
    __syncthreads();
    bq_wave_put<bq_op_max>(low, shw);
    bq_wave_put<bq_op_max>(lown, shw2);
    __syncthreads();
    if (threadIdx.x == 0)
        mr_nu_next(P, c, cc, first, uv, ui, mr_waves_max(shw), nv, ni, mr_waves_max(shw2), ui < 0 ? -1 : rows[ui], ni < 0 ? -1 : rows[ni]);
    if (!bq_last_block(&P.glob->ticket, (unsigned int)live)) return;
    mr_resolve_last<2>(P, shl, false);
}

// ---- the start gradient ---------------------------------------------------------------------------------------------------------------
struct ms_ent {   // a nonzero of a column's folded start: b, and where its row stands in the ascending union of all columns' rows
    double b;
    int u, pad_;
};
struct ms_tab {
    const ms_ent *ent;    // every column's nonzeros, ascending by row, column by column
    const int2 *range;    // per (batch, column): the entries of the column whose rows the batch holds
    const int *has;       // per column: whether it has a nonzero at all (one without keeps lin's bits)
    double *acc;          // the accumulators between two batches, laid out like G (full form: one per ROW, c n + t)
    int u0;               // the batch's first row of the union: row u of the union sits in slot req_out[u - u0]
};

// full columns: the grid of mr_update_kernel; `last`: the union is used up, G = lin + s acc (the product exact, one rounded add)
__global__ __launch_bounds__(RSMO_T) void mr_start_kernel(mr_dev P, ms_tab S, int batch, int last) {
    const int c = blockIdx.y;
    const int2 rg = S.range[(int64_t)batch * P.k + c];
    if (!S.has[c] || (rg.x == rg.y && !last)) return;
    const int64_t t = (int64_t)blockIdx.x * RSMO_T + threadIdx.x;
    if (t >= P.n) return;
    double acc = S.acc[(int64_t)c * P.n + t];
    for (int e = rg.x; e < rg.y; ++e) {
        const ms_ent en = S.ent[e];
        const int slot = P.req_out[en.u - S.u0];
        const double kv = P.cache[(int64_t)(slot < 0 ? 0 : slot) * P.pitch + t];
        const double prod = kv * en.b;
        acc = acc + prod;
    }
    if (!last) {
        S.acc[(int64_t)c * P.n + t] = acc;
        return;
    }
    double *G = P.G + (int64_t)c * P.N;
    const double *y = P.y + (int64_t)c * P.N;
    for (int64_t v = t; v < P.N; v += P.n) {
        const double signed_acc = y[v] * acc;
        G[v] = G[v] + signed_acc;
    }
}

// row lists: the flat grid of ml_update_kernel, a thread's PER accumulators in registers across the batch
template <int PER>
__global__ __launch_bounds__(RSMO_T) void ml_start_kernel(mr_dev P, ms_tab S, int batch, int last) {
    const int2 wk = P.work[blockIdx.x];
    const int c = wk.x;
    const int2 rg = S.range[(int64_t)batch * P.k + c];
    if (!S.has[c] || (rg.x == rg.y && !last)) return;
    const ml_info in = P.info[c];
    const int q0 = wk.y + PER * (int)threadIdx.x;
    if (q0 >= in.m) return;
    int r_t[PER];
    double acc[PER];
    ml_load<PER>(P.rows + in.off + q0, r_t);
    ml_load<PER>(S.acc + in.off + q0, acc);
    for (int e = rg.x; e < rg.y; ++e) {
        const ms_ent en = S.ent[e];
        const int slot = P.req_out[en.u - S.u0];
        const double *row = P.cache + (int64_t)(slot < 0 ? 0 : slot) * P.pitch;
        double kv[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) kv[u] = row[r_t[u]];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const double prod = kv[u] * en.b;
            acc[u] = acc[u] + prod;
        }
    }
    double *out = S.acc + in.off + q0;
    if (last) {   // (a pad position follows its column's last row; nobody reads it)
        double g_t[PER], y_t[PER];
        out = P.G + in.off + q0;
        ml_load<PER>(out, g_t);
        ml_load<PER>(P.y + in.off + q0, y_t);
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const double signed_acc = y_t[u] * acc[u];
            acc[u] = g_t[u] + signed_acc;
        }
    }
#pragma unroll
    for (int u = 0; u < PER / 2; ++u) reinterpret_cast<bq_d2 *>(out)[u] = (bq_d2){acc[2 * u], acc[2 * u + 1]};
}

}   // namespace
