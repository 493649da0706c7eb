// Panel-free SMO (bq_rsmo_*, bcqp.h): libsvm's WSS2 decomposition on kernel rows made on demand from the k-major image a streamed
// problem keeps on the device.  The scalar rules — set predicates, the WSS2 score, the two-variable update with its clipping, the rho
// pieces, the cache's victim rule — are bq_rsmo_step.h, shared with the host check; this file holds the row kernel, the cache and
// the two launches of a step.
//
// A step:
//   rsmo_select_kernel  row i (computed into its cache slot, or read from it on a hit); every thread scores the variables of its
//                       column as partner j (WSS2); the last workgroup picks j, resolves the slot of its row, and one thread makes
//                       the two-variable update of alpha (K_ij travels with the candidate).
//   rsmo_update_kernel  row j (computed or read); G_t += Q_it d_i + Q_jt d_j; per-workgroup maxima over I_up and I_low; the last
//                       workgroup picks the next i, evaluates the stop test and resolves the slot of the next row.
// Values travel between workgroups through the partials and the ticket of bq_reduce.h or across a kernel boundary, never otherwise:
// the control block, the cache's tables and alpha are written by the last workgroup of a launch only, after every other workgroup
// has taken the ticket (and so has finished reading them), and read by the next launch.  All arg-max / arg-min combines are
// (value, larger index): a total order, so the result does not depend on the grid.  Once `finished` is up, launches return at once.
//
// bq_rsmo_create_general takes the dual as data (signs, linear term, boxes, a start alpha0 and a rule).  Under BQ_RSMO_RULE_NU the step
// is libsvm's Solver_NU, still two launches: the update kernel picks one maximal violator per sign (ip, in) and resolves both rows'
// slots, the select kernel makes the missing rows (both in one pass over the image when both miss), scores every variable against
// the row of its own sign, picks j and with it i = ip or in, and resolves row j keeping both others.
//
// A row is one ascending-feature fma chain per column over the image, x_i staged in LDS; <x_i, x_t> and <x_t, x_i> are the same
// chain (fma(a, b, c) = fma(b, a, c)) and the two norms are added to each other first, so K[i][t] and K[t][i] have the same bits, and
// a row has the same bits whenever it is computed: nothing in a trajectory depends on the cache.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "bq_common.h"
#include "bq_gram_image.h"
#include "bq_reduce.h"
#include "bq_rsmo_step.h"

namespace {

constexpr int RSMO_T = 256;        // threads per workgroup = columns per workgroup (the slice)
constexpr int RSMO_XCHUNK = 512;   // features of x_i staged at a time

struct rsmo_ctl {
    long long steps, cap, clock, hits, misses, filled;
    int i, slot_i, hit_i;    // the pending selection: variable i, the slot of its row, whether the slot already holds the row
    int j, slot_j, hit_j;    // the partner chosen by the select kernel
    int finished;            // 0 running, 1 optimal, 2 stopped at the cap
    int last_i, last_j;      // the pair of the last update
    int req_slot, req_hit;   // bq_rsmo_rows: the slot of the requested row
    unsigned int ticket;
    double gmax, gmax2, d_i, d_j, y_i, y_j;
    // BQ_RSMO_RULE_NU: i / slot_i / hit_i / gmax / gmax2 are the positive side's (ip, Gmaxp, Gmaxp2), these the negative side's
    int i2, slot_2, hit_2;
    int slot_u;              // the slot of the row of the i that the select kernel paired with j (slot_i or slot_2)
    double gmaxn, gmaxn2;
};

struct rsmo_dev {
    int64_t n, N, mp, d, R, pitch;
    const double *At, *a2, *X;
    double gamma, coef0, tol;
    int degree;
    double *alpha, *G, *y, *Cb, *QD;   // N, N, N (signs), N (boxes), n
    double *cache;                     // R x pitch
    int *slot_of, *row_of;             // n: slot of a row or -1; R: row of a slot or -1
    long long *stamp;                  // R: clock of the last use, 0 = never
    rsmo_ctl *ctl;
    double *part_v, *part_k, *part_w;  // per workgroup: candidate value, its K_it, the I_low maximum
    long long *part_i;                 // ... and its index
    double *part_v2, *part_w2;         // BQ_RSMO_RULE_NU: the negative side's candidate and maximum
    long long *part_i2;
    double *rowbuf;                    // n: a row on its way to the host
};

// ---- the kernel map (bq_gram_image.h / bq_exp.h) on one inner product ------------------------------------------------------------
template <int KIND, int DEG>
__device__ __forceinline__ double rsmo_map(const rsmo_dev &P, double dot, double a_r, double a_t, bool diag) {
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

// K[r][t] for the column t of this thread (0 beyond n); called by every thread of the workgroup (barriers inside)
template <int KIND, int DEG>
__device__ __forceinline__ double rsmo_row_value(const rsmo_dev &P, int64_t r, int64_t t, double *xs) {
    double acc = 0.0;
    for (int64_t k0 = 0; k0 < P.d; k0 += RSMO_XCHUNK) {
        const int len = (int)(P.d - k0 < RSMO_XCHUNK ? P.d - k0 : RSMO_XCHUNK);
        __syncthreads();
        for (int k = threadIdx.x; k < len; k += RSMO_T) xs[k] = P.X[r * P.d + k0 + k];
        __syncthreads();
        if (t < P.n) {
            const double *col = P.At + k0 * P.mp + t;
#pragma unroll 8
            for (int k = 0; k < len; ++k) acc = fma(xs[k], col[(int64_t)k * P.mp], acc);
        }
    }
    if (t >= P.n) return 0.0;
    const bool rbf = KIND == BQ_KERNEL_RBF;
    return rsmo_map<KIND, DEG>(P, acc, rbf ? P.a2[r] : 0.0, rbf ? P.a2[t] : 0.0, t == r);
}

// K[ra][t] and K[rb][t] in ONE pass over the image: both x rows staged in LDS, each column value loaded once and fed to two ascending
// fma chains — each chain is rsmo_row_value's own, so each row has the bits it has when it is computed alone
template <int KIND, int DEG>
__device__ __forceinline__ void rsmo_row_value2(const rsmo_dev &P, int64_t ra, int64_t rb, int64_t t, double *xs, double *ka, double *kb) {
    double acc_a = 0.0, acc_b = 0.0;
    double *xa = xs, *xb = xs + RSMO_XCHUNK;
    for (int64_t k0 = 0; k0 < P.d; k0 += RSMO_XCHUNK) {
        const int len = (int)(P.d - k0 < RSMO_XCHUNK ? P.d - k0 : RSMO_XCHUNK);
        __syncthreads();
        for (int k = threadIdx.x; k < len; k += RSMO_T) {
            xa[k] = P.X[ra * P.d + k0 + k];
            xb[k] = P.X[rb * P.d + k0 + k];
        }
        __syncthreads();
        if (t < P.n) {
            const double *col = P.At + k0 * P.mp + t;
#pragma unroll 8
            for (int k = 0; k < len; ++k) {
                const double x = col[(int64_t)k * P.mp];
                acc_a = fma(xa[k], x, acc_a);
                acc_b = fma(xb[k], x, acc_b);
            }
        }
    }
    *ka = *kb = 0.0;
    if (t >= P.n) return;
    const bool rbf = KIND == BQ_KERNEL_RBF;
    *ka = rsmo_map<KIND, DEG>(P, acc_a, rbf ? P.a2[ra] : 0.0, rbf ? P.a2[t] : 0.0, t == ra);
    *kb = rsmo_map<KIND, DEG>(P, acc_b, rbf ? P.a2[rb] : 0.0, rbf ? P.a2[t] : 0.0, t == rb);
}

// ---- (value, index, rider) picks over a workgroup: every thread receives the winner --------------------------------------------------
struct rsmo_min_order {
    static __device__ __forceinline__ bool before(double va, long long ia, double vb, long long ib) { return bq_rsmo_min_before(va, ia, vb, ib); }
};
struct rsmo_max_order {
    static __device__ __forceinline__ bool before(double va, long long ia, double vb, long long ib) { return bq_rsmo_max_before(va, ia, vb, ib); }
};
struct rsmo_victim_order {
    static __device__ __forceinline__ bool before(long long va, long long ia, long long vb, long long ib) { return bq_rsmo_victim_before(va, ia, vb, ib); }
};
template <typename V>
struct rsmo_pick_smem {
    V v[RSMO_T / 64];
    long long i[RSMO_T / 64];
    double k[RSMO_T / 64];
};
template <typename ORDER, typename V>
__device__ __forceinline__ void rsmo_block_pick(V &v, long long &idx, double &rider, rsmo_pick_smem<V> &sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const V v2 = __shfl_down(v, off, 64);
        const long long i2 = __shfl_down(idx, off, 64);
        const double k2 = __shfl_down(rider, off, 64);
        if (ORDER::before(v2, i2, v, idx)) {
            v = v2;
            idx = i2;
            rider = k2;
        }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        sh.v[threadIdx.x >> 6] = v;
        sh.i[threadIdx.x >> 6] = idx;
        sh.k[threadIdx.x >> 6] = rider;
    }
    __syncthreads();
    v = sh.v[0];
    idx = sh.i[0];
    rider = sh.k[0];
#pragma unroll
    for (int w = 1; w < RSMO_T / 64; ++w)
        if (ORDER::before(sh.v[w], sh.i[w], v, idx)) {
            v = sh.v[w];
            idx = sh.i[w];
            rider = sh.k[w];
        }
}

// ---- the cache: slot of row r, called by every thread of ONE workgroup (the last of a launch, or a one-workgroup launch) -----------
// Hit: the stamp is refreshed.  Miss: the victim of bq_rsmo_step.h (slots never used go first, in order), never `keep` or `keep2`.
// *hit is uniform over the workgroup; the tables are written by thread 0 after every thread has read them.
__device__ __forceinline__ int rsmo_resolve(const rsmo_dev &P, int64_t r, int keep, int *hit, rsmo_pick_smem<long long> &sh,
                                            int keep2 = -1) {
    rsmo_ctl *c = P.ctl;
    const int have = P.slot_of[r];
    const long long filled = c->filled;
    long long victim = -1;
    if (have < 0) {
        if (filled < P.R) {
            victim = filled;
        } else {
            long long best = 0;
            double rider = 0.0;
            for (int64_t s = threadIdx.x; s < P.R; s += RSMO_T) {
                const long long st = P.stamp[s];
                if (s != keep && s != keep2 && bq_rsmo_victim_before(st, s, best, victim)) {
                    best = st;
                    victim = s;
                }
            }
            rsmo_block_pick<rsmo_victim_order>(best, victim, rider, sh);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long now = c->clock + 1;
        c->clock = now;
        if (have >= 0) {
            P.stamp[have] = now;
            c->hits += 1;
        } else {
            const int old = P.row_of[victim];
            if (old >= 0) P.slot_of[old] = -1;
            P.row_of[victim] = (int)r;
            P.slot_of[r] = (int)victim;
            P.stamp[victim] = now;
            if (filled < P.R) c->filled = filled + 1;
            c->misses += 1;
        }
    }
    *hit = have >= 0 ? 1 : 0;
    __syncthreads();   // a second resolve of the same tail reads the tables thread 0 has just written
    return have >= 0 ? have : (int)victim;
}
// a request for the row a slot of the step in hand already holds: a hit, nothing to look up (thread 0 of the last workgroup)
__device__ __forceinline__ void rsmo_touch(const rsmo_dev &P, int slot) {
    P.stamp[slot] = ++P.ctl->clock;
    P.ctl->hits += 1;
}

__device__ __forceinline__ int64_t rsmo_row_of(const rsmo_dev &P, int v) { return v < 0 ? -1 : (v >= P.n ? v - P.n : v); }

// ---- launch 1 of a step: row i, WSS2 candidates, j, the pair update -----------------------------------------------------------------
// BQ_RSMO_RULE_NU: the rows of ip and in (one pass over the image makes both when both miss); a variable is scored against the row
// of its own sign; i is ip or in according to y_j, and the slot of row j is resolved keeping both.
template <int KIND, int DEG, int RULE>
__global__ __launch_bounds__(RSMO_T) void rsmo_select_kernel(rsmo_dev P) {
    constexpr bool NU = RULE == BQ_RSMO_RULE_NU;
    rsmo_ctl *c = P.ctl;
    if (c->finished) return;
    __shared__ double xs[NU ? 2 * RSMO_XCHUNK : RSMO_XCHUNK];
    __shared__ rsmo_pick_smem<double> sh;
    __shared__ rsmo_pick_smem<long long> shl;
    const int i = c->i, slot_i = c->slot_i, hit_i = c->hit_i;
    const double gmax = c->gmax;
    const int64_t r = rsmo_row_of(P, i);
    const int64_t t = (int64_t)blockIdx.x * RSMO_T + threadIdx.x;
    double *row = P.cache + (int64_t)(slot_i < 0 ? 0 : slot_i) * P.pitch;
    double k = 0.0;
    // NU: the negative side
    const int i2 = NU ? c->i2 : -1, slot_2 = NU ? c->slot_2 : -1;
    const double gmaxn = NU ? c->gmaxn : -BQ_RSMO_INF;
    const int64_t r2 = rsmo_row_of(P, i2);
    double k2 = 0.0;
    if (!NU) {
        if (hit_i) {
            if (t < P.n) k = row[t];
        } else {
            k = rsmo_row_value<KIND, DEG>(P, r, t, xs);
            if (t < P.n) row[t] = k;
        }
    } else {
        double *row2 = P.cache + (int64_t)(slot_2 < 0 ? 0 : slot_2) * P.pitch;
        const bool make = i >= 0 && !hit_i, make2 = i2 >= 0 && !c->hit_2 && r2 != r;   // (ip and in on one row: one slot, made once)
        if (make && make2) {
            rsmo_row_value2<KIND, DEG>(P, r, r2, t, xs, &k, &k2);
            if (t < P.n) {
                row[t] = k;
                row2[t] = k2;
            }
        } else if (make) {
            k = rsmo_row_value<KIND, DEG>(P, r, t, xs);
            if (t < P.n) row[t] = k;
        } else if (make2) {
            k2 = rsmo_row_value<KIND, DEG>(P, r2, t, xs);
            if (t < P.n) row2[t] = k2;
        }
        if (t < P.n) {
            if (i >= 0 && !make) k = row[t];
            if (i2 >= 0 && !make2) k2 = r2 == r ? k : row2[t];
        }
    }
    const double qd_i = i >= 0 ? P.QD[r] : 0.0, qd_2 = i2 >= 0 ? P.QD[r2] : 0.0;
    double bv = BQ_RSMO_INF, bk = 0.0;
    long long bi = -1;
    if (t < P.n) {
        const double qd_t = P.QD[t];
        for (int64_t v = t; v < P.N; v += P.n) {   // BQ_SVR: the variables t and t + n share the row
            const double y_t = P.y[v];
            if (!bq_rsmo_in_low(y_t, P.alpha[v], P.Cb[v])) continue;
            bool ok;
            const double sc = NU ? bq_rsmo_nu_score(y_t, P.G[v], gmax, qd_i, k, gmaxn, qd_2, k2, qd_t, &ok)
                                 : bq_rsmo_score(gmax, y_t, P.G[v], qd_i, qd_t, k, &ok);
            if (ok && bq_rsmo_min_before(sc, v, bv, bi)) {
                bv = sc;
                bi = v;
                bk = NU && y_t < 0.0 ? k2 : k;
            }
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
        const long long i2b = bq_part_get(&P.part_i[b]);
        const double k2b = bq_part_get(&P.part_k[b]);
        if (bq_rsmo_min_before(v2, i2b, bv, bi)) {
            bv = v2;
            bi = i2b;
            bk = k2b;
        }
    }
    rsmo_block_pick<rsmo_min_order>(bv, bi, bk, sh);
    if (bi < 0) {   // no partner: libsvm's Gmin_idx == -1
        if (threadIdx.x == 0) c->finished = 1;
        return;
    }
    const int j = (int)bi;
    const int64_t rj = j >= P.n ? j - P.n : j;
    // the i of the pair: NU takes the maximal violator of j's sign
    const bool neg = NU && P.y[j] < 0.0;
    const int iu = neg ? i2 : i, slot_u = neg ? slot_2 : slot_i;
    const int64_t ru = neg ? r2 : r;
    int slot_j = slot_u, hit_j = 1;
    if (rj == ru) {   // BQ_SVR: the two variables of one row
        if (threadIdx.x == 0) rsmo_touch(P, slot_u);
    } else {
        slot_j = rsmo_resolve(P, rj, slot_i, &hit_j, shl, slot_2);
    }
    if (threadIdx.x == 0) {
        const double y_i = P.y[iu], y_j = P.y[j];
        const double old_i = P.alpha[iu], old_j = P.alpha[j];
        double a_i = old_i, a_j = old_j;
        bq_rsmo_pair_update(y_i, y_j, P.G[iu], P.G[j], neg ? qd_2 : qd_i, P.QD[rj], bk, P.Cb[iu], P.Cb[j], &a_i, &a_j);
        P.alpha[iu] = a_i;
        P.alpha[j] = a_j;
        c->d_i = a_i - old_i;
        c->d_j = a_j - old_j;
        c->y_i = y_i;
        c->y_j = y_j;
        c->j = j;
        c->slot_j = slot_j;
        c->hit_j = hit_j;
        c->slot_u = slot_u;
        c->last_i = iu;
        c->last_j = j;
    }
}

// ---- launch 2 of a step: row j, the gradient, the next i and the stop test (first: the selection before the first step) -------------
// BQ_RSMO_RULE_NU: the next ip and in, the four maxima, the two-sided stop test, and the slots of both rows (the second resolve keeps
// the first row's slot; a side without a violator requests nothing; ip and in on one row use one slot, the second request a hit).
template <int KIND, int DEG, int RULE>
__global__ __launch_bounds__(RSMO_T) void rsmo_update_kernel(rsmo_dev P, int first) {
    constexpr bool NU = RULE == BQ_RSMO_RULE_NU;
    rsmo_ctl *c = P.ctl;
    if (c->finished) return;
    __shared__ double xs[RSMO_XCHUNK];
    __shared__ rsmo_pick_smem<double> sh;
    __shared__ rsmo_pick_smem<long long> shl;
    __shared__ double shw[RSMO_T / 64], shw2[RSMO_T / 64];
    const int64_t t = (int64_t)blockIdx.x * RSMO_T + threadIdx.x;
    double g[2] = {0.0, 0.0};
    if (t < P.n) {
        g[0] = P.G[t];
        if (P.N > P.n) g[1] = P.G[t + P.n];
    }
    if (!first) {
        const int j = c->j, slot_i = c->slot_u, slot_j = c->slot_j, hit_j = c->hit_j;
        const int64_t rj = j >= P.n ? j - P.n : j;
        const double d_i = c->d_i, d_j = c->d_j, y_i = c->y_i, y_j = c->y_j;
        double *row_j = P.cache + (int64_t)slot_j * P.pitch;
        const double *row_i = P.cache + (int64_t)slot_i * P.pitch;
        double kj = 0.0;
        if (hit_j) {
            if (t < P.n) kj = row_j[t];
        } else {
            kj = rsmo_row_value<KIND, DEG>(P, rj, t, xs);
            if (t < P.n) row_j[t] = kj;
        }
        if (t < P.n) {
            const double ki = row_i[t];
            int h = 0;
            for (int64_t v = t; v < P.N; v += P.n, ++h) {
                const double y_t = P.y[v];
                const double s_i = y_i * y_t, s_j = y_j * y_t;   // +-1: exact
                const double q_i = s_i * ki, q_j = s_j * kj;
                g[h] = bq_rsmo_grad(g[h], q_i, d_i, q_j, d_j);
                P.G[v] = g[h];
            }
        }
    }
    // PLAIN: (uv, ui) the arg-max over I_up, low the maximum over I_low; NU: the same of the positive sign, (nv, ni) / lown of the negative
    double uv = -BQ_RSMO_INF, rider = 0.0, low = -BQ_RSMO_INF;
    long long ui = -1;
    double nv = -BQ_RSMO_INF, lown = -BQ_RSMO_INF;
    long long ni = -1;
    if (t < P.n) {
        int h = 0;
        for (int64_t v = t; v < P.N; v += P.n, ++h) {
            const double y_t = P.y[v], a = P.alpha[v], C = P.Cb[v];
            const bool second = NU && y_t < 0.0;
            if (bq_rsmo_in_up(y_t, a, C)) {
                const double val = bq_rsmo_up_value(y_t, g[h]);
                if (second) {
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
                if (second)
                    lown = fmax(lown, bq_rsmo_low_value(y_t, g[h]));
                else
                    low = fmax(low, bq_rsmo_low_value(y_t, g[h]));
            }
        }
    }
    rsmo_block_pick<rsmo_max_order>(uv, ui, rider, sh);
    if (NU) rsmo_block_pick<rsmo_max_order>(nv, ni, rider, sh);
    bq_wave_put<bq_op_max>(low, shw);
    if (NU) bq_wave_put<bq_op_max>(lown, shw2);
    __syncthreads();
    if (threadIdx.x == 0) {
        double w = shw[0];
        for (int q = 1; q < RSMO_T / 64; ++q) w = fmax(w, shw[q]);
        bq_part_put(&P.part_v[blockIdx.x], uv);
        bq_part_put(&P.part_i[blockIdx.x], ui);
        bq_part_put(&P.part_w[blockIdx.x], w);
        if (NU) {
            double w2 = shw2[0];
            for (int q = 1; q < RSMO_T / 64; ++q) w2 = fmax(w2, shw2[q]);
            bq_part_put(&P.part_v2[blockIdx.x], nv);
            bq_part_put(&P.part_i2[blockIdx.x], ni);
            bq_part_put(&P.part_w2[blockIdx.x], w2);
        }
    }
    if (!bq_last_block(&c->ticket, gridDim.x)) return;
    uv = -BQ_RSMO_INF;
    ui = -1;
    low = -BQ_RSMO_INF;
    nv = -BQ_RSMO_INF;
    ni = -1;
    lown = -BQ_RSMO_INF;
    for (unsigned int b = threadIdx.x; b < gridDim.x; b += RSMO_T) {
        const double v2 = bq_part_get(&P.part_v[b]);
        const long long i2 = bq_part_get(&P.part_i[b]);
        if (bq_rsmo_max_before(v2, i2, uv, ui)) {
            uv = v2;
            ui = i2;
        }
        low = fmax(low, bq_part_get(&P.part_w[b]));
        if (NU) {
            const double v3 = bq_part_get(&P.part_v2[b]);
            const long long i3 = bq_part_get(&P.part_i2[b]);
            if (bq_rsmo_max_before(v3, i3, nv, ni)) {
                nv = v3;
                ni = i3;
            }
            lown = fmax(lown, bq_part_get(&P.part_w2[b]));
        }
    }
    rsmo_block_pick<rsmo_max_order>(uv, ui, rider, sh);
    if (NU) rsmo_block_pick<rsmo_max_order>(nv, ni, rider, sh);
    __syncthreads();
    bq_wave_put<bq_op_max>(low, shw);
    if (NU) bq_wave_put<bq_op_max>(lown, shw2);
    __syncthreads();
    low = shw[0];
    for (int q = 1; q < RSMO_T / 64; ++q) low = fmax(low, shw[q]);
    if (NU) {
        lown = shw2[0];
        for (int q = 1; q < RSMO_T / 64; ++q) lown = fmax(lown, shw2[q]);
    }
    const long long steps = c->steps + (first ? 0 : 1);
    int fin = 0;
    if (NU ? ((ui < 0 && ni < 0) || bq_rsmo_nu_stop(uv, low, nv, lown, P.tol)) : (ui < 0 || bq_rsmo_stop(uv, low, P.tol)))
        fin = 1;
    else if (steps >= c->cap)
        fin = 2;
    int slot = -1, hit = 0, slot2 = -1, hit2 = 0;
    if (!fin) {
        const int64_t r = rsmo_row_of(P, (int)ui), r2 = rsmo_row_of(P, (int)ni);
        if (ui >= 0) slot = rsmo_resolve(P, r, -1, &hit, shl);
        if (NU && ni >= 0) {
            if (r2 == r) {
                slot2 = slot;
                hit2 = 1;
                if (threadIdx.x == 0) rsmo_touch(P, slot);
            } else {
                slot2 = rsmo_resolve(P, r2, slot, &hit2, shl);
            }
        }
    }
    if (threadIdx.x == 0) {
        c->steps = steps;
        c->gmax = uv;
        c->gmax2 = low;
        c->i = (int)ui;
        c->slot_i = slot;
        c->hit_i = hit;
        c->finished = fin;
        if (NU) {
            c->gmaxn = nv;
            c->gmaxn2 = lown;
            c->i2 = (int)ni;
            c->slot_2 = slot2;
            c->hit_2 = hit2;
        }
    }
}

// ---- QD = diag(K), by the row's arithmetic --------------------------------------------------------------------------------------
template <int KIND, int DEG>
__global__ __launch_bounds__(RSMO_T) void rsmo_diag_kernel(rsmo_dev P) {
    const int64_t t = (int64_t)blockIdx.x * RSMO_T + threadIdx.x;
    if (t >= P.n) return;
    double acc = 0.0;
    const double *col = P.At + t;
    for (int64_t k = 0; k < P.d; ++k) {
        const double x = col[k * P.mp];
        acc = fma(x, x, acc);
    }
    const double a = KIND == BQ_KERNEL_RBF ? P.a2[t] : 0.0;
    P.QD[t] = rsmo_map<KIND, DEG>(P, acc, a, a, true);
}

// ---- bq_rsmo_rows: one requested row through the cache ------------------------------------------------------------------------------
__global__ __launch_bounds__(RSMO_T) void rsmo_request_kernel(rsmo_dev P, int64_t r) {
    __shared__ rsmo_pick_smem<long long> shl;
    rsmo_ctl *c = P.ctl;
    const int pending = c->finished ? -1 : c->slot_i, computed = c->hit_i;
    const int pending2 = c->finished ? -1 : c->slot_2, computed2 = c->hit_2;   // BQ_RSMO_RULE_NU: the negative side's row (else -1)
    int hit = 0;
    const int slot = rsmo_resolve(P, r, pending, &hit, shl, pending2);
    if (threadIdx.x == 0) {
        // the pending row's slot is assigned before the select kernel fills it: a request for that row fills it here
        if (slot == pending && !computed) {
            hit = 0;
            c->hit_i = 1;
        } else if (slot >= 0 && slot == pending2 && !computed2) {
            hit = 0;
            c->hit_2 = 1;
        }
        c->req_slot = slot;
        c->req_hit = hit;
    }
}
template <int KIND, int DEG>
__global__ __launch_bounds__(RSMO_T) void rsmo_fill_kernel(rsmo_dev P, int64_t r) {
    __shared__ double xs[RSMO_XCHUNK];
    const rsmo_ctl *c = P.ctl;
    const int64_t t = (int64_t)blockIdx.x * RSMO_T + threadIdx.x;
    double *row = P.cache + (int64_t)c->req_slot * P.pitch;
    double k = 0.0;
    if (c->req_hit) {
        if (t < P.n) k = row[t];
    } else {
        k = rsmo_row_value<KIND, DEG>(P, r, t, xs);
        if (t < P.n) row[t] = k;
    }
    if (t < P.n) P.rowbuf[t] = k;
}

template <int K, int D>
struct rsmo_kind {
    static constexpr int kind = K, deg = D;
};
template <typename F>
int rsmo_dispatch(const bq_problem *p, F f) {
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

}   // namespace

struct bq_rsmo {
    bq_problem *p = nullptr;
    int rule = BQ_RSMO_RULE_PLAIN;
    bq_owner mem;
    rsmo_dev P = {};
    unsigned int nblk = 0;
    std::vector<double> y, Cb;   // host copies for calculate_rho
    rsmo_ctl host = {};
};

extern "C" int bq_rsmo_destroy(bq_rsmo *s) {
    if (s == nullptr) return BQ_OK;
    bq_problem *p = s->p;
    hipSetDevice(p->ctx->device);
    hipStreamSynchronize(p->ctx->stream);
    delete s;
    bq_problem_unref(p);
    return BQ_OK;
}

static int rsmo_read_ctl(bq_rsmo *s) {
    bq_ctx *c = s->p->ctx;
    BQ_HIP(hipMemcpyAsync(&s->host, s->P.ctl, sizeof(rsmo_ctl), hipMemcpyDeviceToHost, c->stream));
    BQ_HIP(hipStreamSynchronize(c->stream));
    return BQ_OK;
}

// the start gradient: G_v = lin_v + s_v (K b)_row(v), the product exact (s = +-1), one rounded add
static __global__ __launch_bounds__(RSMO_T) void rsmo_start_kernel(rsmo_dev P, const double *Kb) {
    const int64_t t = (int64_t)blockIdx.x * RSMO_T + threadIdx.x;
    if (t >= P.n) return;
    const double kb = Kb[t];
    for (int64_t v = t; v < P.N; v += P.n) {
        const double signed_kb = P.y[v] * kb;
        P.G[v] = P.G[v] + signed_kb;
    }
}

template <typename KD>
static void rsmo_launch_update(KD, int rule, const rsmo_dev &P, unsigned int nblk, hipStream_t st, int first) {
    if (rule == BQ_RSMO_RULE_NU)
        rsmo_update_kernel<KD::kind, KD::deg, BQ_RSMO_RULE_NU><<<nblk, RSMO_T, 0, st>>>(P, first);
    else
        rsmo_update_kernel<KD::kind, KD::deg, BQ_RSMO_RULE_PLAIN><<<nblk, RSMO_T, 0, st>>>(P, first);
}
template <typename KD>
static void rsmo_launch_select(KD, int rule, const rsmo_dev &P, unsigned int nblk, hipStream_t st) {
    if (rule == BQ_RSMO_RULE_NU)
        rsmo_select_kernel<KD::kind, KD::deg, BQ_RSMO_RULE_NU><<<nblk, RSMO_T, 0, st>>>(P);
    else
        rsmo_select_kernel<KD::kind, KD::deg, BQ_RSMO_RULE_PLAIN><<<nblk, RSMO_T, 0, st>>>(P);
}

// The start.  alpha = alpha0 and G0 = lin + s o (K b) folded to N, b_t the sum over the variables of row t of s_v alpha0_v.  b = 0
// (alpha0 = 0, or nu-SVR's equal halves): G0 = lin with lin's bits and no product.  Otherwise G0 is ONE streamed Gram product of the
// problem (bq_panel_product -> bq_stream_sym_product, the product bq_problem_matvec runs), computed once: it does not depend on the
// cache or on how the run is cut, and a trajectory is reproducible from (rows, alpha0, G0).  libsvm's own start sums alpha_i Q_i in
// ascending i; this one differs from that in rounding only (the tile order of the product).
extern "C" int bq_rsmo_create_general(bq_problem *p, int rule, int64_t N, const double *signs, const double *lin, const double *boxes,
                                      const double *alpha0, double tol, int64_t max_steps, int64_t cache_rows, bq_rsmo **out) {
    BQ_ARG(p && signs && lin && boxes && alpha0 && out, "NULL argument");
    BQ_ARG(rule == BQ_RSMO_RULE_PLAIN || rule == BQ_RSMO_RULE_NU, "rule must be BQ_RSMO_RULE_PLAIN or BQ_RSMO_RULE_NU");
    BQ_ARG(p->kernel >= 0 && p->streamed && p->stream_img != nullptr && p->ctx->world == 1,
           "the row-based SMO needs a kernel-built streamed problem (BQ_STREAM) on a single-rank context");
    BQ_ARG(tol > 0.0, "tol must be > 0");
    BQ_ARG(max_steps >= 0, "max_steps must be >= 0 (0: libsvm's cap)");
    BQ_ARG(cache_rows == 0 || cache_rows >= 2, "cache_rows must be 0 (automatic) or >= 2");
    BQ_ARG(rule != BQ_RSMO_RULE_NU || cache_rows != 2, "a Solver_NU step holds three rows: cache_rows must be 0 or >= 3");
    const int64_t n = p->n;
    BQ_ARG(N == n || N == 2 * n, "N must be n or 2n");
    BQ_ARG(N < ((int64_t)1 << 31), "the dual dimension must stay below 2^31");
    bool pos = false, neg = false, zero_b = true;
    for (int64_t v = 0; v < N; ++v) {
        BQ_ARG(std::isfinite(boxes[v]) && boxes[v] > 0.0, "every box must be finite and > 0");
        BQ_ARG(signs[v] == 1.0 || signs[v] == -1.0, "signs must be +1 / -1");
        BQ_ARG(N == n || signs[v] == (v < n ? 1.0 : -1.0), "the signs of 2n variables must be [+1 ..; -1 ..]");
        BQ_ARG(std::isfinite(lin[v]), "the linear term must be finite");
        BQ_ARG(alpha0[v] >= 0.0 && alpha0[v] <= boxes[v], "the start must lie in its box");
        pos |= signs[v] > 0.0;
        neg |= signs[v] < 0.0;
    }
    BQ_ARG(rule != BQ_RSMO_RULE_NU || (pos && neg), "Solver_NU needs both signs");
    // b, folded to the rows
    std::vector<double> b((size_t)n);
    for (int64_t t = 0; t < n; ++t) {
        double acc = signs[t] * alpha0[t];
        if (N > n) acc = acc + signs[t + n] * alpha0[t + n];
        b[t] = acc;
        zero_b &= acc == 0.0;
    }
    bq_ctx *c = p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    bq_rsmo *s = new bq_rsmo();
    s->p = p;
    s->rule = rule;
    p->refs += 1;
    rsmo_dev &P = s->P;
    int64_t dp = 0;
    bq_stream_image_view(p->stream_img, &P.At, &P.a2, &P.mp, &dp);
    P.n = n;
    P.N = N;
    P.d = p->d;
    P.X = p->X;
    P.gamma = p->gamma;
    P.coef0 = p->coef0;
    P.degree = p->degree;
    P.tol = tol;
    P.pitch = P.mp;
    s->nblk = (unsigned int)((n + RSMO_T - 1) / RSMO_T);
    // host images of the dual for calculate_rho
    s->y.assign(signs, signs + N);
    s->Cb.assign(boxes, boxes + N);
    auto fail = [&](hipError_t e, const char *what) {
        bq_set_error("%s failed: %s", what, hipGetErrorString(e));
        hipStreamSynchronize(c->stream);
        bq_rsmo_destroy(s);
        return e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
    };
    hipError_t e = hipSuccess;
    e = s->mem.dev(&P.alpha, (size_t)N);
    if (e == hipSuccess) e = s->mem.dev(&P.G, (size_t)N);
    if (e == hipSuccess) e = s->mem.dev(&P.y, (size_t)N);
    if (e == hipSuccess) e = s->mem.dev(&P.Cb, (size_t)N);
    if (e == hipSuccess) e = s->mem.dev(&P.QD, (size_t)n);
    if (e == hipSuccess) e = s->mem.dev(&P.slot_of, (size_t)n);
    if (e == hipSuccess) e = s->mem.dev(&P.rowbuf, (size_t)n);
    if (e == hipSuccess) e = s->mem.dev(&P.part_v, (size_t)s->nblk);
    if (e == hipSuccess) e = s->mem.dev(&P.part_k, (size_t)s->nblk);
    if (e == hipSuccess) e = s->mem.dev(&P.part_w, (size_t)s->nblk);
    if (e == hipSuccess) e = s->mem.dev(&P.part_i, (size_t)s->nblk);
    if (e == hipSuccess) e = s->mem.dev(&P.part_v2, (size_t)s->nblk);
    if (e == hipSuccess) e = s->mem.dev(&P.part_w2, (size_t)s->nblk);
    if (e == hipSuccess) e = s->mem.dev(&P.part_i2, (size_t)s->nblk);
    e = bq_dev_zeroed(e, s->mem, &P.ctl, 1, c->stream);
    if (e != hipSuccess) return fail(e, "the row-based SMO's vectors");
    // the cache: the rows asked for, or what half of the free memory holds, at most n
    int64_t R = cache_rows;
    if (R == 0) {
        size_t free_b = 0, total_b = 0;
        if ((e = hipMemGetInfo(&free_b, &total_b)) != hipSuccess) return fail(e, "hipMemGetInfo");
        R = (int64_t)(free_b / 2 / (sizeof(double) * (size_t)P.pitch));
        const int64_t least = rule == BQ_RSMO_RULE_NU ? 3 : 2;
        if (R < least) R = least;
    }
    if (R > n) R = n;
    P.R = R;
    if ((e = s->mem.dev(&P.cache, (size_t)R * (size_t)P.pitch)) != hipSuccess) return fail(e, "the row cache");
    if ((e = s->mem.dev(&P.row_of, (size_t)R)) != hipSuccess) return fail(e, "the row cache");
    e = bq_dev_zeroed(e, s->mem, &P.stamp, (size_t)R, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(P.slot_of, 0xFF, sizeof(int) * (size_t)n, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(P.row_of, 0xFF, sizeof(int) * (size_t)R, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(P.alpha, alpha0, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(P.G, lin, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(P.y, s->y.data(), sizeof(double) * (size_t)N, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(P.Cb, s->Cb.data(), sizeof(double) * (size_t)N, hipMemcpyHostToDevice, c->stream);
    rsmo_ctl c0 = {};
    c0.cap = max_steps > 0 ? (long long)max_steps : std::max<long long>(10000000LL, 100LL * (long long)N);   // libsvm's max_iter
    c0.cap = (long long)bq_hook_value("rsmo_max_steps", (double)c0.cap);
    c0.i = c0.j = c0.i2 = c0.last_i = c0.last_j = -1;
    c0.slot_i = c0.slot_j = c0.slot_2 = c0.slot_u = -1;
    c0.gmax = c0.gmax2 = c0.gmaxn = c0.gmaxn2 = -INFINITY;
    if (e == hipSuccess) e = hipMemcpyAsync(P.ctl, &c0, sizeof(c0), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return fail(e, "the row-based SMO's start");
    int rc = BQ_OK;
    if (!zero_b) {   // K b through the problem's own product buffers: w (ld, zero beyond n) in, s out
        e = hipMemsetAsync(p->w, 0, sizeof(double) * (size_t)p->ld, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(p->w, b.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return fail(e, "the row-based SMO's start");
        rc = bq_panel_product(p, false, p->w, nullptr);
        if (rc == BQ_OK) {
            rsmo_start_kernel<<<s->nblk, RSMO_T, 0, c->stream>>>(P, p->s);
            if ((e = hipGetLastError()) != hipSuccess) return fail(e, "the row-based SMO's start gradient");
        }
    }
    if (rc == BQ_OK)
        rc = rsmo_dispatch(p, [&](auto kd) {
            rsmo_diag_kernel<decltype(kd)::kind, decltype(kd)::deg><<<s->nblk, RSMO_T, 0, c->stream>>>(P);
            rsmo_launch_update(kd, rule, P, s->nblk, c->stream, 1);
        });
    if (rc == BQ_OK && (e = hipGetLastError()) != hipSuccess) return fail(e, "the row-based SMO's first selection");
    if (rc == BQ_OK) rc = rsmo_read_ctl(s);   // (b, c0 and the caller's vectors are read by then: nothing is in flight afterwards)
    if (rc != BQ_OK) {
        hipStreamSynchronize(c->stream);
        bq_rsmo_destroy(s);
        return rc;
    }
    *out = s;
    return BQ_OK;
}

// libsvm's C-SVC / epsilon-SVR duals: the general entry with alpha0 = 0 (G0 = p, no product) and the task's signs and linear term
extern "C" int bq_rsmo_create(bq_problem *p, int task, const double *y, const double *Cw, double epsilon, double tol,
                              int64_t cache_rows, bq_rsmo **out) {
    BQ_ARG(p && y && Cw && out, "NULL argument");
    BQ_ARG(task == BQ_SVC || task == BQ_SVR, "task must be BQ_SVC or BQ_SVR");
    BQ_ARG(p->kernel >= 0 && p->streamed && p->stream_img != nullptr && p->ctx->world == 1,
           "the row-based SMO needs a kernel-built streamed problem (BQ_STREAM) on a single-rank context");
    BQ_ARG(tol > 0.0, "tol must be > 0");
    BQ_ARG(epsilon >= 0.0, "epsilon must be >= 0");
    BQ_ARG(cache_rows == 0 || cache_rows >= 2, "cache_rows must be 0 (automatic) or >= 2");
    const int64_t n = p->n, N = task == BQ_SVR ? 2 * n : n;
    BQ_ARG(N < ((int64_t)1 << 31), "the dual dimension must stay below 2^31");
    bool pos = false, neg = false;
    for (int64_t t = 0; t < n; ++t) {
        BQ_ARG(std::isfinite(Cw[t]) && Cw[t] > 0.0, "every box must be finite and > 0");
        if (task == BQ_SVC) {
            BQ_ARG(y[t] == 1.0 || y[t] == -1.0, "labels must be +1 / -1");
            pos |= y[t] > 0.0;
            neg |= y[t] < 0.0;
        } else {
            BQ_ARG(std::isfinite(y[t]), "targets must be finite");
        }
    }
    BQ_ARG(task != BQ_SVC || (pos && neg), "both classes are needed");
    std::vector<double> signs((size_t)N), lin((size_t)N), boxes((size_t)N), zero((size_t)N, 0.0);
    for (int64_t t = 0; t < n; ++t) {
        if (task == BQ_SVC) {
            signs[t] = y[t];
            boxes[t] = Cw[t];
            lin[t] = -1.0;
        } else {
            signs[t] = 1.0;
            signs[t + n] = -1.0;
            boxes[t] = boxes[t + n] = Cw[t];
            lin[t] = epsilon - y[t];
            lin[t + n] = epsilon + y[t];
        }
    }
    return bq_rsmo_create_general(p, BQ_RSMO_RULE_PLAIN, N, signs.data(), lin.data(), boxes.data(), zero.data(), tol, 0, cache_rows, out);
}

extern "C" int bq_rsmo_run(bq_rsmo *s, int64_t max_steps, int64_t *steps, int *finished) {
    BQ_ARG(s && steps && finished, "NULL argument");
    BQ_ARG(max_steps > 0, "max_steps must be > 0");
    bq_ctx *c = s->p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    if (!s->host.finished) {
        const rsmo_dev &P = s->P;
        BQ_TRY(rsmo_dispatch(s->p, [&](auto kd) {
            for (int64_t k = 0; k < max_steps; ++k) {
                rsmo_launch_select(kd, s->rule, P, s->nblk, c->stream);
                rsmo_launch_update(kd, s->rule, P, s->nblk, c->stream, 0);
            }
        }));
        BQ_HIP(hipGetLastError());
        BQ_TRY(rsmo_read_ctl(s));
    }
    *steps = s->host.steps;
    *finished = s->host.finished;
    return BQ_OK;
}

extern "C" int bq_rsmo_get(bq_rsmo *s, int what, double *out) {
    BQ_ARG(s && out, "NULL argument");
    BQ_ARG(what >= BQ_RSMO_ALPHAS && what <= BQ_RSMO_NU_SCALARS, "what");
    BQ_ARG(what != BQ_RSMO_NU_SCALARS || s->rule == BQ_RSMO_RULE_NU, "BQ_RSMO_NU_SCALARS needs a BQ_RSMO_RULE_NU solver");
    bq_ctx *c = s->p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    const rsmo_dev &P = s->P;
    if (what == BQ_RSMO_ALPHAS || what == BQ_RSMO_GRADIENT) {
        BQ_HIP(hipMemcpyAsync(out, what == BQ_RSMO_ALPHAS ? P.alpha : P.G, sizeof(double) * (size_t)P.N, hipMemcpyDeviceToHost, c->stream));
        BQ_HIP(hipStreamSynchronize(c->stream));
        return BQ_OK;
    }
    BQ_TRY(rsmo_read_ctl(s));
    if (what == BQ_RSMO_STATS) {
        out[0] = (double)s->host.hits;
        out[1] = (double)s->host.misses;
        out[2] = (double)P.R;
        return BQ_OK;
    }
    // calculate_rho in libsvm's order, on the host: one pass over the two vectors, once per fit
    std::vector<double> a((size_t)P.N), g((size_t)P.N);
    BQ_HIP(hipMemcpyAsync(a.data(), P.alpha, sizeof(double) * (size_t)P.N, hipMemcpyDeviceToHost, c->stream));
    BQ_HIP(hipMemcpyAsync(g.data(), P.G, sizeof(double) * (size_t)P.N, hipMemcpyDeviceToHost, c->stream));
    BQ_HIP(hipStreamSynchronize(c->stream));
    if (s->rule == BQ_RSMO_RULE_NU) {
        bq_rsmo_nu_rho nu;
        for (int64_t t = 0; t < P.N; ++t) bq_rsmo_nu_rho_add(&nu, s->y[t], a[t], s->Cb[t], g[t]);
        double rho = 0.0, r = 0.0;
        bq_rsmo_nu_rho_value(&nu, &rho, &r);
        out[0] = rho;
        if (what == BQ_RSMO_NU_SCALARS) {
            out[1] = r;
            out[2] = bq_rsmo_nu_gap(s->host.gmax, s->host.gmax2);
            out[3] = bq_rsmo_nu_gap(s->host.gmaxn, s->host.gmaxn2);
            out[4] = (double)s->host.last_i;
            out[5] = (double)s->host.last_j;
            out[6] = (double)s->host.steps;
            return BQ_OK;
        }
    } else {
        bq_rsmo_rho rho;
        for (int64_t t = 0; t < P.N; ++t) bq_rsmo_rho_add(&rho, s->y[t], a[t], s->Cb[t], g[t]);
        out[0] = bq_rsmo_rho_value(&rho);
    }
    out[1] = s->host.gmax;
    out[2] = s->host.gmax2;
    out[3] = (double)s->host.last_i;
    out[4] = (double)s->host.last_j;
    out[5] = (double)s->host.steps;
    return BQ_OK;
}

extern "C" int bq_rsmo_rows(bq_rsmo *s, int m, const int64_t *idx, double *out) {
    BQ_ARG(s && idx && out, "NULL argument");
    BQ_ARG(m >= 1, "m must be >= 1");
    const rsmo_dev &P = s->P;
    for (int q = 0; q < m; ++q) BQ_ARG(idx[q] >= 0 && idx[q] < P.n, "a requested row lies outside the problem");
    bq_ctx *c = s->p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    for (int q = 0; q < m; ++q) {
        const int64_t r = idx[q];
        rsmo_request_kernel<<<1, RSMO_T, 0, c->stream>>>(P, r);
        BQ_TRY(rsmo_dispatch(s->p, [&](auto kd) {
            rsmo_fill_kernel<decltype(kd)::kind, decltype(kd)::deg><<<s->nblk, RSMO_T, 0, c->stream>>>(P, r);
        }));
        BQ_HIP(hipGetLastError());
        BQ_HIP(hipMemcpyAsync(out + (size_t)q * (size_t)P.n, P.rowbuf, sizeof(double) * (size_t)P.n, hipMemcpyDeviceToHost, c->stream));
        BQ_HIP(hipStreamSynchronize(c->stream));   // rowbuf is free for the next row
    }
    return rsmo_read_ctl(s);
}
