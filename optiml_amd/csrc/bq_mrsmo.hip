// Batched panel-free SMO (bq_mrsmo_*, bcqp.h): k columns of libsvm's WSS2 decomposition (the scalar rules of bq_rsmo_step.h; rule
// BQ_RSMO_RULE_PLAIN here, BQ_RSMO_RULE_NU and the start gradient of nonzero starts in bq_mrsmo_nu.h) on ONE streamed problem, ONE cache of kernel rows, and kernel rows made 16 at a time by fp64 MFMA.
// A row of K does not depend on the labels: every column asks for rows of the same matrix, so the rows all columns need in a phase
// of a step are resolved together (bq_mrsmo_cache.h) and the missing ones are made in one pass over the k-major image.
//
// A step of all live columns is four launches:
//   mr_rows_kernel    the missing rows i      grid: column blocks of MR_COLS
//   mr_select_kernel  WSS2 partner j, update  grid: (slices of RSMO_T columns) x (columns of the batch)
//   mr_rows_kernel    the missing rows j
//   mr_update_kernel  gradient, next i, stop  grid: (slices) x (columns)
// select / update are bq_rsmo.hip's with the row read from its slot.  Per column the slices meet at the column's ticket
// (bq_reduce.h) and the last one takes the column's decision; the columns meet at the solver's ticket and the last one resolves the
// cache for all of them and writes the miss list the next mr_rows_kernel reads — the host never sees it.  What crosses workgroups
// inside a launch (partials, the requested rows) travels as agent-scope atomics; everything else is written by the last workgroup
// of one launch and read by the next launch.  A column that has finished launches nothing but returning workgroups.
//
// The row-block kernel.  A workgroup owns MR_COLS = 256 columns of the image, a wave 64 of them as four independent 16 x 16
// accumulator tiles: lane (c = lane & 15, q = lane >> 4) feeds tile j the column 4 c + j of the wave's 64, so one k-row of the image
// is read by a lane as 32 contiguous bytes and by 16 lanes as 512, and each value loaded feeds all 16 rows.  A is the up to 16
// requested rows of X, staged in LDS in fragment order (As[kb][lane] = x_{row(lane & 15)}[4 kb + (lane >> 4)]), MR_KC features at a
// time, zero where the group has fewer than 16 rows or the feature index is beyond d - 1 (the image is not read there either).
// v_mfma_f64_16x16x4_f64 keeps rows and columns of D apart, and every element is the same ascending sequence of k-blocks: the bits
// of K[r][t] depend on x_r, x_t and d only, and (r, t) and (t, r) are the same products in the same order.
//
// The row-list form (bq_mrsmo_create_lists).  Column c is the dual on the m_c rows of its strictly ascending list (a class pair of
// one-vs-one: about 2 n / classes rows); its variables are the POSITIONS 0 .. m_c - 1, every tie breaks on the position, so the
// column is the solver run on K[rows][:, rows].  The state of all columns is packed, each column at an offset that is a multiple of
// ML_PAD, with the list beside it as int32; requests, the cache, the row-block kernel and QD stay in global rows, so a row made
// for one pair serves every pair of its class.  ml_select_kernel / ml_update_kernel replace launches 2 and 4:
//   - the grid is FLAT: workgroup w reads (column, first position) from a work table the host builds at create; the launch is
//     sum_c ceil(m_c / slice) workgroups, none outside a list, where the (slices of n) x (columns) grid above would launch
//     45 n / 256 workgroups for the 45 pairs of ten classes to touch 45 * 2 n / 10 positions;
//   - a workgroup owns a slice of RSMO_T * PER consecutive positions, a thread PER consecutive ones: alpha / G / y / Cb come in as
//     8 PER contiguous bytes each and the list as 4 PER, and the only scattered reads are the kernel values k = row[list[q]] (and
//     QD[list[q]], n doubles that stay in L2).  Per-workgroup cost — the block pick, the partials, the fence and the ticket — is
//     paid once per RSMO_T * PER positions instead of once per 256;
//   - a column's ticket counts its own slices, the solver's ticket the live columns, as above.
// Scans inside a thread go through the same total orders as the picks, so no result depends on PER or on the work table.
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#include "bq_common.h"
#include "bq_gram_image.h"
#include "bq_mrsmo_cache.h"
#include "bq_reduce.h"
#include "bq_rsmo_map.h"
#include "bq_rsmo_pick.h"
#include "bq_rsmo_step.h"

namespace {

constexpr int MR_COLS = 256;   // image columns per workgroup of the row-block kernel (4 waves x 4 tiles x 16)
constexpr int MR_G = 16;       // rows per pass: the MFMA's M
constexpr int MR_KC = 256;     // features of the 16 rows staged at a time (32 KiB of LDS)
constexpr int MR_REQ = 1024;   // requests per resolution (the tables of the last workgroup): columns of a batch, rows of a bq_mrsmo_rows call
constexpr int ML_PER = 8;      // list form: positions per thread, MR_SLICE = RSMO_T * ML_PER per workgroup; 8 measured best of 2, 4, 8
                               // (profiles/ovo_smo_rows/; hook mrsmo_list_per switches a solver to 2 or 4)
constexpr int ML_PAD = 8;      // list form: a column's packed offset is a multiple of this, so the widest thread's loads are aligned

struct mr_col {   // a column's control block
    long long steps;
    int i, slot_i;          // the pending selection and the slot of its row
    int j, slot_j;          // the partner the select kernel chose
    int finished;           // 0 running, 1 optimal, 2 stopped at the cap
    int last_i, last_j;
    unsigned int ticket;
    double gmax, gmax2, d_i, d_j, y_i, y_j;
    // BQ_RSMO_RULE_NU: i / slot_i / gmax / gmax2 are the positive side's (ip, Gmaxp, Gmaxp2), these the negative side's
    int i2, slot_2;
    int slot_u, pad_;       // the slot of the row of the i that the select kernel paired with j (slot_i or slot_2)
    double gmaxn, gmaxn2;
};
struct mr_glob {
    bq_mrsmo_cache cache;
    long long cap;
    int live;     // columns still running: the arrivals of the solver's ticket
    int n_miss;   // the miss list's length
    unsigned int ticket;
};
struct ml_info {   // a column of the list form
    int64_t off;   // where its state and its list start in the packed arrays (a multiple of ML_PAD)
    int m;         // its positions
    int nsl;       // its slices: the arrivals of its ticket
    int part0;     // its first partial
    int pad_;
};
struct mr_dev {
    int64_t n, N, mp, d, pitch;
    int k;
    const double *At, *a2, *X;
    double gamma, coef0, tol;
    int degree;
    double *alpha, *G, *y, *Cb;   // k x N
    double *QD;                   // n
    double *cache;                // R x pitch
    mr_col *col;                  // k
    mr_glob *glob;
    int *req_row;                 // k: the row each column asks for in the phase in hand, -1: none; BQ_RSMO_RULE_NU: 3 k, the j
                                  // phase's request of column c at [c], the i phase's two (ip, in) at [k + 2 c], [k + 2 c + 1]
    int nreq;                     // requests per column in the i phase = rows a live column waits for between steps: 1, NU 2
    int *miss_row, *miss_slot;    // MR_REQ: the distinct missing rows and their slots
    int *req_in, *req_out;        // MR_REQ: bq_mrsmo_rows' requests and their slots
    int *res_req, *res_slot, *res_pin;   // MR_REQ each: the tables of a resolution, touched by the launch's last workgroup only
    double *part_v, *part_k, *part_w;   // k x nblk
    long long *part_i;
    double *part_v2, *part_w2;          // BQ_RSMO_RULE_NU: the negative side's candidate and maximum
    long long *part_i2;
    // the list form: alpha / G / y / Cb are packed at info[c].off instead of c N, N is 0
    const int *rows;        // the lists, packed like the state; the pad positions of a column repeat its last row
    const ml_info *info;    // k
    const int2 *work;       // per workgroup of ml_select / ml_update: (column, first position of its slice)
};
// The tables of a resolution (requests, their slots, the pins) live in global memory, not in LDS: one workgroup of a launch uses
// them, and 12 KiB of LDS in every workgroup of the (slices x columns) grid would be carried for nothing.  That workgroup writes
// them, passes a barrier and reads them back; nobody else touches them inside the launch.
struct mr_par {   // bq_mrsmo_resolve over the threads of one workgroup
    rsmo_pick_smem<long long> &sh;
    __device__ __forceinline__ int tid() const { return threadIdx.x; }
    __device__ __forceinline__ int size() const { return RSMO_T; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ void pick(long long *best, long long *victim) const {
        double rider = 0.0;
        rsmo_block_pick<rsmo_victim_order>(*best, *victim, rider, sh);
    }
};

// ---- the row-block kernel ---------------------------------------------------------------------------------------------------------
template <int KIND, int DEG>
__global__ __launch_bounds__(RSMO_T) void mr_rows_kernel(mr_dev P) {
    const int n_miss = P.glob->n_miss;
    if (n_miss == 0) return;
    __shared__ double As[(MR_KC / 4) * 64];
    const int tid = threadIdx.x, lane = tid & 63, kq = lane >> 4;
    const int64_t c4 = (int64_t)blockIdx.x * MR_COLS + (tid >> 6) * 64 + 4 * (lane & 15);   // this lane's columns c4 .. c4 + 3
    const bool active = c4 < P.mp;   // wave-uniform: mp is a multiple of 128
    const double *bp = P.At + (active ? c4 : 0);
    for (int g0 = 0; g0 < n_miss; g0 += MR_G) {
        const int cnt = n_miss - g0 < MR_G ? n_miss - g0 : MR_G;
        bq_d4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = (bq_d4){0.0, 0.0, 0.0, 0.0};
        for (int64_t k0 = 0; k0 < P.d; k0 += MR_KC) {
            const int len = (int)(P.d - k0 < MR_KC ? P.d - k0 : MR_KC), nkb = (len + 3) / 4, nfull = len / 4;
            __syncthreads();
            for (int e = tid; e < nkb * 64; e += RSMO_T) {
                const int r = e & 15;
                const int64_t kk = k0 + 4 * (e >> 6) + ((e & 63) >> 4);
                As[e] = r < cnt && kk < P.d ? P.X[(int64_t)P.miss_row[g0 + r] * P.d + kk] : 0.0;
            }
            __syncthreads();
            if (active) {
                const double *b = bp + (k0 + kq) * P.mp;
                auto block = [&](int kb) {   // one k-block of 4: 32 bytes of the image per lane, four independent MFMAs
                    const double a = As[kb * 64 + lane];
                    const bq_d2 lo = *reinterpret_cast<const bq_d2 *>(b), hi = *reinterpret_cast<const bq_d2 *>(b + 2);
                    b += 4 * P.mp;
                    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, lo.x, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, lo.y, acc[1], 0, 0, 0);
                    acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, hi.x, acc[2], 0, 0, 0);
                    acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, hi.y, acc[3], 0, 0, 0);
                };
                int kb = 0;
                for (; kb + 4 <= nfull; kb += 4) {   // four blocks' loads go out before the first MFMA waits
#pragma unroll
                    for (int u = 0; u < 4; ++u) block(kb + u);
                }
                for (; kb < nfull; ++kb) block(kb);
                if (nfull < nkb) {   // the k-block that crosses d: zero operands beyond row d - 1, which is not read
                    const double a = As[nfull * 64 + lane];
                    bq_d2 lo = (bq_d2){0.0, 0.0}, hi = (bq_d2){0.0, 0.0};
                    if (k0 + 4 * nfull + kq < P.d) {
                        lo = *reinterpret_cast<const bq_d2 *>(b);
                        hi = *reinterpret_cast<const bq_d2 *>(b + 2);
                    }
                    acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, lo.x, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, lo.y, acc[1], 0, 0, 0);
                    acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, hi.x, acc[2], 0, 0, 0);
                    acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, hi.y, acc[3], 0, 0, 0);
                }
            }
        }
        if (!active) continue;
        // D: column lane & 15 of each tile (= column c4 + j), rows (lane >> 4) + 4 v of the group
        const bool rbf = KIND == BQ_KERNEL_RBF;
        double a_t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a_t[j] = rbf ? P.a2[c4 + j] : 0.0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int r = kq + 4 * v;
            if (r >= cnt) continue;
            const int64_t rr = P.miss_row[g0 + r];
            double *out = P.cache + (int64_t)P.miss_slot[g0 + r] * P.pitch + c4;
            const double a_r = rbf ? P.a2[rr] : 0.0;
            double val[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) val[j] = rsmo_map<KIND, DEG>(P, acc[j][v], a_r, a_t[j], c4 + j == rr);
            if (c4 + 3 < P.n) {
                *reinterpret_cast<bq_d2 *>(out) = (bq_d2){val[0], val[1]};
                *reinterpret_cast<bq_d2 *>(out + 2) = (bq_d2){val[2], val[3]};
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c4 + j < P.n) out[j] = val[j];
            }
        }
    }
}

// QD = diag(K) with the row-block kernel's arithmetic: a wave takes 16 columns as both operands of the same k-blocks
template <int KIND, int DEG>
__global__ __launch_bounds__(RSMO_T) void mr_diag_kernel(mr_dev P) {
    const int lane = threadIdx.x & 63, kq = lane >> 4, c = lane & 15;
    const int64_t t = ((int64_t)blockIdx.x * (RSMO_T / 64) + (threadIdx.x >> 6)) * 16 + c;
    if (t - c >= P.mp) return;
    bq_d4 acc = (bq_d4){0.0, 0.0, 0.0, 0.0};
    for (int64_t k0 = 0; k0 < P.d; k0 += 4) {
        const double a = k0 + kq < P.d ? P.At[(k0 + kq) * P.mp + t] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc, 0, 0, 0);
    }
    const double a2 = KIND == BQ_KERNEL_RBF ? P.a2[t] : 0.0;
#pragma unroll
    for (int v = 0; v < 4; ++v)
        if (kq + 4 * v == c && t < P.n) P.QD[t] = rsmo_map<KIND, DEG>(P, acc[v], a2, a2, true);
}

// ---- the resolution of a phase: every thread of the launch's LAST workgroup --------------------------------------------------------
// phase_j: the rows j are asked for while the rows i of the same columns are still to be read (pins).  NQ: the requests (and the
// pinned rows) per column of the i phase — 1, Solver_NU 2 (ip, in), whose i-phase requests live behind the k of the j phase.
template <int NQ = 1>
__device__ __forceinline__ void mr_resolve_last(const mr_dev &P, rsmo_pick_smem<long long> &pick, bool phase_j) {
    const int nq = phase_j ? 1 : NQ, m = nq * P.k;
    const int *req_row = P.req_row + (NQ > 1 && !phase_j ? P.k : 0);
    for (int e = threadIdx.x; e < m; e += RSMO_T) P.res_req[e] = bq_part_get(&req_row[e]);
    for (int e = threadIdx.x; e < NQ * P.k; e += RSMO_T) {
        const int c = e / NQ;
        P.res_pin[e] = phase_j && bq_part_get(&P.req_row[c]) >= 0 ? (e % NQ ? P.col[c].slot_2 : P.col[c].slot_i) : -1;
    }
    __syncthreads();
    mr_par par{pick};
    bq_mrsmo_resolve(&P.glob->cache, phase_j ? NQ * P.k : 0, P.res_pin, m, P.res_req, P.res_slot, P.miss_row, P.miss_slot, &P.glob->n_miss,
                     par);
    __syncthreads();
    for (int c = threadIdx.x; c < P.k; c += RSMO_T) {
        if (phase_j) {
            P.col[c].slot_j = P.res_slot[c];
        } else {
            P.col[c].slot_i = P.res_slot[NQ * c];
            if (NQ > 1) P.col[c].slot_2 = P.res_slot[NQ * c + 1];
        }
    }
    if (threadIdx.x == 0) {
        int live = 0;
        for (int c = 0; c < P.k; ++c) {   // a column that goes on asks for a row in either phase
            bool asks = false;
            for (int h = 0; h < nq; ++h) asks = asks || P.res_req[nq * c + h] >= 0;
            live += asks ? 1 : 0;
        }
        P.glob->live = live;
    }
}

// ---- launch 2 of a step: WSS2 candidates against row i, j, the pair update ----------------------------------------------------------
__global__ __launch_bounds__(RSMO_T) void mr_select_kernel(mr_dev P) {
    const int c = blockIdx.y;
    mr_col *cc = &P.col[c];
    const int live = P.glob->live;
    if (cc->finished) return;
    __shared__ rsmo_pick_smem<double> sh;
    __shared__ rsmo_pick_smem<long long> shl;
    const double *alpha = P.alpha + (int64_t)c * P.N, *G = P.G + (int64_t)c * P.N, *y = P.y + (int64_t)c * P.N,
                 *Cb = P.Cb + (int64_t)c * P.N;
    const int i = cc->i, slot_i = cc->slot_i;
    const double gmax = cc->gmax;
    const int64_t r = i >= P.n ? i - P.n : i;
    const int64_t t = (int64_t)blockIdx.x * RSMO_T + threadIdx.x;
    const double *row = P.cache + (int64_t)(slot_i < 0 ? 0 : slot_i) * P.pitch;
    const double k = t < P.n ? row[t] : 0.0;
    const double qd_i = P.QD[r];
    double bv = BQ_RSMO_INF, bk = 0.0;
    long long bi = -1;
    if (t < P.n) {
        const double qd_t = P.QD[t];
        for (int64_t v = t; v < P.N; v += P.n) {   // 2n variables: t and t + n share the row
            const double y_t = y[v];
            if (!bq_rsmo_in_low(y_t, alpha[v], Cb[v])) continue;
            bool ok;
            const double sc = bq_rsmo_score(gmax, y_t, G[v], qd_i, qd_t, k, &ok);
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
        int req = -1;
        if (bi < 0) {   // no partner: libsvm's Gmin_idx == -1
            cc->finished = 1;
        } else {
            const int j = (int)bi;
            const int64_t rj = j >= P.n ? j - P.n : j;
            double *al = P.alpha + (int64_t)c * P.N;
            const double y_i = y[i], y_j = y[j];
            const double old_i = al[i], old_j = al[j];
            double a_i = old_i, a_j = old_j;
            bq_rsmo_pair_update(y_i, y_j, G[i], G[j], qd_i, P.QD[rj], bk, Cb[i], Cb[j], &a_i, &a_j);
            al[i] = a_i;
            al[j] = a_j;
            cc->d_i = a_i - old_i;
            cc->d_j = a_j - old_j;
            cc->y_i = y_i;
            cc->y_j = y_j;
            cc->j = j;
            cc->last_i = i;
            cc->last_j = j;
            req = (int)rj;
        }
        bq_part_put(&P.req_row[c], req);
    }
    if (!bq_last_block(&P.glob->ticket, (unsigned int)live)) return;
    mr_resolve_last(P, shl, true);
}

// ---- launch 4 of a step: the gradient, the next i and the stop test (first: the selection before the first step) --------------------
__global__ __launch_bounds__(RSMO_T) void mr_update_kernel(mr_dev P, int first) {
    const int c = blockIdx.y;
    mr_col *cc = &P.col[c];
    const int live = P.glob->live;
    if (cc->finished) return;
    __shared__ rsmo_pick_smem<double> sh;
    __shared__ rsmo_pick_smem<long long> shl;
    __shared__ double shw[RSMO_T / 64];
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
        const double ki = P.cache[(int64_t)(cc->slot_i < 0 ? 0 : cc->slot_i) * P.pitch + t];
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
    double uv = -BQ_RSMO_INF, rider = 0.0, low = -BQ_RSMO_INF;
    long long ui = -1;
    if (t < P.n) {
        int h = 0;
        for (int64_t v = t; v < P.N; v += P.n, ++h) {
            const double y_t = y[v], a = alpha[v], C = Cb[v];
            if (bq_rsmo_in_up(y_t, a, C)) {
                const double val = bq_rsmo_up_value(y_t, g[h]);
                if (bq_rsmo_max_before(val, v, uv, ui)) {
                    uv = val;
                    ui = v;
                }
            }
            if (bq_rsmo_in_low(y_t, a, C)) low = fmax(low, bq_rsmo_low_value(y_t, g[h]));
        }
    }
    rsmo_block_pick<rsmo_max_order>(uv, ui, rider, sh);
    bq_wave_put<bq_op_max>(low, shw);
    __syncthreads();
    const int64_t pb = (int64_t)c * gridDim.x;
    if (threadIdx.x == 0) {
        double w = shw[0];
        for (int q = 1; q < RSMO_T / 64; ++q) w = fmax(w, shw[q]);
        bq_part_put(&P.part_v[pb + blockIdx.x], uv);
        bq_part_put(&P.part_i[pb + blockIdx.x], ui);
        bq_part_put(&P.part_w[pb + blockIdx.x], w);
    }
    if (!bq_last_block(&cc->ticket, gridDim.x)) return;
    uv = -BQ_RSMO_INF;
    ui = -1;
    low = -BQ_RSMO_INF;
    for (unsigned int b = threadIdx.x; b < gridDim.x; b += RSMO_T) {
        const double v2 = bq_part_get(&P.part_v[pb + b]);
        const long long i2 = bq_part_get(&P.part_i[pb + b]);
        if (bq_rsmo_max_before(v2, i2, uv, ui)) {
            uv = v2;
            ui = i2;
        }
        low = fmax(low, bq_part_get(&P.part_w[pb + b]));
    }
    rsmo_block_pick<rsmo_max_order>(uv, ui, rider, sh);
    __syncthreads();
    bq_wave_put<bq_op_max>(low, shw);
    __syncthreads();
    if (threadIdx.x == 0) {
        low = shw[0];
        for (int q = 1; q < RSMO_T / 64; ++q) low = fmax(low, shw[q]);
        const long long steps = cc->steps + (first ? 0 : 1);
        int fin = 0;
        if (ui < 0 || bq_rsmo_stop(uv, low, P.tol))
            fin = 1;
        else if (steps >= P.glob->cap)
            fin = 2;
        cc->steps = steps;
        cc->gmax = uv;
        cc->gmax2 = low;
        cc->i = (int)ui;
        cc->finished = fin;
        bq_part_put(&P.req_row[c], fin ? -1 : (int)(ui >= P.n ? ui - P.n : ui));
    }
    if (!bq_last_block(&P.glob->ticket, (unsigned int)live)) return;
    mr_resolve_last(P, shl, false);
}

// ---- the row-list form of launches 2 and 4 ------------------------------------------------------------------------------------------
// a thread's PER consecutive doubles / list entries: 16-byte loads at an address that is a multiple of 8 PER / 4 PER bytes
template <int PER>
__device__ __forceinline__ void ml_load(const double *p, double (&v)[PER]) {
#pragma unroll
    for (int u = 0; u < PER / 2; ++u) {
        const bq_d2 t = reinterpret_cast<const bq_d2 *>(p)[u];
        v[2 * u] = t.x;
        v[2 * u + 1] = t.y;
    }
}
template <int PER>
__device__ __forceinline__ void ml_load(const int *p, int (&v)[PER]) {
    if constexpr (PER == 2) {
        const int2 t = *reinterpret_cast<const int2 *>(p);
        v[0] = t.x;
        v[1] = t.y;
    } else {
#pragma unroll
        for (int u = 0; u < PER / 4; ++u) {
            const int4 t = reinterpret_cast<const int4 *>(p)[u];
            v[4 * u] = t.x;
            v[4 * u + 1] = t.y;
            v[4 * u + 2] = t.z;
            v[4 * u + 3] = t.w;
        }
    }
}

template <int PER>
__global__ __launch_bounds__(RSMO_T) void ml_select_kernel(mr_dev P) {
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
    const int i = cc->i, slot_i = cc->slot_i;
    const double gmax = cc->gmax;
    const double *row = P.cache + (int64_t)(slot_i < 0 ? 0 : slot_i) * P.pitch;
    const double qd_i = P.QD[rows[i]];
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
        for (int e = 0; e < PER; ++e) {   // the gathers go out together
            k_t[e] = row[r_t[e]];
            qd_t[e] = P.QD[r_t[e]];
        }
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            if (q0 + e >= in.m || !bq_rsmo_in_low(y_t[e], a_t[e], C_t[e])) continue;
            bool ok;
            const double sc = bq_rsmo_score(gmax, y_t[e], g_t[e], qd_i, qd_t[e], k_t[e], &ok);
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
        int req = -1;
        if (bi < 0) {   // no partner: libsvm's Gmin_idx == -1
            cc->finished = 1;
        } else {
            const int j = (int)bi, rj = rows[j];
            double *al = P.alpha + in.off;
            const double y_i = y[i], y_j = y[j];
            const double old_i = al[i], old_j = al[j];
            double a_i = old_i, a_j = old_j;
            bq_rsmo_pair_update(y_i, y_j, G[i], G[j], qd_i, P.QD[rj], bk, Cb[i], Cb[j], &a_i, &a_j);
            al[i] = a_i;
            al[j] = a_j;
            cc->d_i = a_i - old_i;
            cc->d_j = a_j - old_j;
            cc->y_i = y_i;
            cc->y_j = y_j;
            cc->j = j;
            cc->last_i = i;
            cc->last_j = j;
            req = rj;
        }
        bq_part_put(&P.req_row[c], req);
    }
    if (!bq_last_block(&P.glob->ticket, (unsigned int)live)) return;
    mr_resolve_last(P, shl, true);
}

template <int PER>
__global__ __launch_bounds__(RSMO_T) void ml_update_kernel(mr_dev P, int first) {
    const int2 wk = P.work[blockIdx.x];
    const int c = wk.x;
    mr_col *cc = &P.col[c];
    const int live = P.glob->live;
    if (cc->finished) return;
    __shared__ rsmo_pick_smem<double> sh;
    __shared__ rsmo_pick_smem<long long> shl;
    __shared__ double shw[RSMO_T / 64];
    const ml_info in = P.info[c];
    const double *alpha = P.alpha + in.off, *y = P.y + in.off, *Cb = P.Cb + in.off;
    double *G = P.G + in.off;
    const int *rows = P.rows + in.off;
    const int q0 = wk.y + PER * (int)threadIdx.x;
    double uv = -BQ_RSMO_INF, rider = 0.0, low = -BQ_RSMO_INF;
    long long ui = -1;
    if (q0 < in.m) {
        double a_t[PER], g_t[PER], y_t[PER], C_t[PER];
        ml_load<PER>(y + q0, y_t);
        ml_load<PER>(G + q0, g_t);
        if (!first) {
            int r_t[PER];
            double ki[PER], kj[PER];
            ml_load<PER>(rows + q0, r_t);
            const double d_i = cc->d_i, d_j = cc->d_j, y_i = cc->y_i, y_j = cc->y_j;
            const double *row_i = P.cache + (int64_t)(cc->slot_i < 0 ? 0 : cc->slot_i) * P.pitch;
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
            if (bq_rsmo_in_up(y_t[e], a_t[e], C_t[e])) {
                const double val = bq_rsmo_up_value(y_t[e], g_t[e]);
                if (bq_rsmo_max_before(val, q0 + e, uv, ui)) {
                    uv = val;
                    ui = q0 + e;
                }
            }
            if (bq_rsmo_in_low(y_t[e], a_t[e], C_t[e])) low = fmax(low, bq_rsmo_low_value(y_t[e], g_t[e]));
        }
    }
    rsmo_block_pick<rsmo_max_order>(uv, ui, rider, sh);
    bq_wave_put<bq_op_max>(low, shw);
    __syncthreads();
    const int64_t pb = in.part0, mine = pb + wk.y / (RSMO_T * PER);
    if (threadIdx.x == 0) {
        double w = shw[0];
        for (int q = 1; q < RSMO_T / 64; ++q) w = fmax(w, shw[q]);
        bq_part_put(&P.part_v[mine], uv);
        bq_part_put(&P.part_i[mine], ui);
        bq_part_put(&P.part_w[mine], w);
    }
    if (!bq_last_block(&cc->ticket, (unsigned int)in.nsl)) return;
    uv = -BQ_RSMO_INF;
    ui = -1;
    low = -BQ_RSMO_INF;
    for (int b = threadIdx.x; b < in.nsl; b += RSMO_T) {
        const double v2 = bq_part_get(&P.part_v[pb + b]);
        const long long i2 = bq_part_get(&P.part_i[pb + b]);
        if (bq_rsmo_max_before(v2, i2, uv, ui)) {
            uv = v2;
            ui = i2;
        }
        low = fmax(low, bq_part_get(&P.part_w[pb + b]));
    }
    rsmo_block_pick<rsmo_max_order>(uv, ui, rider, sh);
    __syncthreads();
    bq_wave_put<bq_op_max>(low, shw);
    __syncthreads();
    if (threadIdx.x == 0) {
        low = shw[0];
        for (int q = 1; q < RSMO_T / 64; ++q) low = fmax(low, shw[q]);
        const long long steps = cc->steps + (first ? 0 : 1);
        int fin = 0;
        if (ui < 0 || bq_rsmo_stop(uv, low, P.tol))
            fin = 1;
        else if (steps >= P.glob->cap)
            fin = 2;
        cc->steps = steps;
        cc->gmax = uv;
        cc->gmax2 = low;
        cc->i = (int)ui;
        cc->finished = fin;
        bq_part_put(&P.req_row[c], fin ? -1 : rows[ui]);
    }
    if (!bq_last_block(&P.glob->ticket, (unsigned int)live)) return;
    mr_resolve_last(P, shl, false);
}

}   // namespace
#include "bq_mrsmo_nu.h"   // Solver_NU's select / update in both forms and the start gradient of nonzero starts
namespace {

// ---- bq_mrsmo_rows: m requested rows through the cache, the rows the live columns wait for pinned ------------------------------------
__global__ __launch_bounds__(RSMO_T) void mr_request_kernel(mr_dev P, int m) {
    __shared__ rsmo_pick_smem<long long> shl;
    for (int q = threadIdx.x; q < MR_REQ; q += RSMO_T) {
        P.res_req[q] = q < m ? P.req_in[q] : -1;
        const int c = q / P.nreq;   // (Solver_NU: a live column waits for the rows of ip and in)
        P.res_pin[q] = c < P.k && !P.col[c].finished ? (q % P.nreq ? P.col[c].slot_2 : P.col[c].slot_i) : -1;
    }
    __syncthreads();
    mr_par par{shl};
    bq_mrsmo_resolve(&P.glob->cache, P.nreq * P.k, P.res_pin, m, P.res_req, P.res_slot, P.miss_row, P.miss_slot, &P.glob->n_miss, par);
    __syncthreads();
    for (int q = threadIdx.x; q < m; q += RSMO_T) P.req_out[q] = P.res_slot[q];
}
// the list is used up: the next step's first pass makes only what its own resolution misses
__global__ void mr_clear_kernel(mr_dev P) { P.glob->n_miss = 0; }

}   // namespace

struct bq_mrsmo {
    bq_problem *p = nullptr;
    int rule = BQ_RSMO_RULE_PLAIN;
    bq_owner mem;
    mr_dev P = {};
    unsigned int nblk = 0;
    int64_t R = 0;
    std::vector<double> y, Cb;   // host copies for calculate_rho (the list form: packed like the device's)
    std::vector<mr_col> host;
    bool done = false;
    // the list form: the columns' packed offsets and lengths, the positions per thread and the flat grid
    std::vector<ml_info> info;
    int per = 0;   // 0: the full-column form
    unsigned int grid = 0;
};

extern "C" int bq_mrsmo_destroy(bq_mrsmo *s) {
    if (s == nullptr) return BQ_OK;
    bq_problem *p = s->p;
    hipSetDevice(p->ctx->device);
    hipStreamSynchronize(p->ctx->stream);
    delete s;
    bq_problem_unref(p);
    return BQ_OK;
}

static int mr_read_cols(bq_mrsmo *s) {
    bq_ctx *c = s->p->ctx;
    BQ_HIP(hipMemcpyAsync(s->host.data(), s->P.col, sizeof(mr_col) * (size_t)s->P.k, hipMemcpyDeviceToHost, c->stream));
    BQ_HIP(hipStreamSynchronize(c->stream));
    s->done = true;
    for (const mr_col &cc : s->host) s->done = s->done && cc.finished != 0;
    return BQ_OK;
}

template <typename KD>
static void mr_launch_rows(KD, const bq_mrsmo *s, hipStream_t st) {
    const unsigned int blocks = (unsigned int)((s->P.mp + MR_COLS - 1) / MR_COLS);
    mr_rows_kernel<KD::kind, KD::deg><<<blocks, RSMO_T, 0, st>>>(s->P);
}

// what both forms of create refuse before they look at a column
static int mr_check(const bq_problem *p, int rule, int k, double tol, int64_t max_steps, int64_t cache_rows) {
    BQ_ARG(rule == BQ_RSMO_RULE_PLAIN || rule == BQ_RSMO_RULE_NU, "rule must be BQ_RSMO_RULE_PLAIN or BQ_RSMO_RULE_NU");
    BQ_ARG(p->kernel >= 0 && p->streamed && p->stream_img != nullptr && p->ctx->world == 1,
           "the row-based SMO needs a kernel-built streamed problem (BQ_STREAM) on a single-rank context");
    BQ_ARG(k >= 1 && k <= MR_REQ, "k must lie in 1 .. 1024");
    BQ_ARG(tol > 0.0, "tol must be > 0");
    BQ_ARG(max_steps >= 0, "max_steps must be >= 0 (0: libsvm's cap)");
    BQ_ARG(cache_rows == 0 || cache_rows >= 2 * (int64_t)k, "cache_rows must be 0 (automatic) or >= 2 k: a step holds two rows per column");
    if (rule == BQ_RSMO_RULE_NU) {
        BQ_ARG(k <= MR_REQ / 2, "Solver_NU asks for two rows per column at once: k must lie in 1 .. 512");
        BQ_ARG(cache_rows == 0 || cache_rows >= 3 * (int64_t)k, "a Solver_NU step holds three rows per column: cache_rows must be 0 or >= 3 k");
    }
    return BQ_OK;
}
static int mr_check_entry(double sign, double lin, double box, double alpha0) {
    BQ_ARG(std::isfinite(box) && box > 0.0, "every box must be finite and > 0");
    BQ_ARG(sign == 1.0 || sign == -1.0, "signs must be +1 / -1");
    BQ_ARG(std::isfinite(lin), "the linear term must be finite");
    BQ_ARG(alpha0 >= 0.0 && alpha0 <= box, "the start must lie in its box");
    return BQ_OK;
}
// a column's nonzeros of the folded start, ascending by row: (row, b)
typedef std::vector<std::pair<int, double>> mr_fold;

// a solver on p with the problem's side of mr_dev filled in
static bq_mrsmo *mr_new(bq_problem *p, int rule, int k, double tol) {
    bq_mrsmo *s = new bq_mrsmo();
    s->p = p;
    s->rule = rule;
    s->P.nreq = rule == BQ_RSMO_RULE_NU ? 2 : 1;
    p->refs += 1;
    mr_dev &P = s->P;
    int64_t dp = 0;
    bq_stream_image_view(p->stream_img, &P.At, &P.a2, &P.mp, &dp);
    P.n = p->n;
    P.k = k;
    P.d = p->d;
    P.X = p->X;
    P.gamma = p->gamma;
    P.coef0 = p->coef0;
    P.degree = p->degree;
    P.tol = tol;
    P.pitch = P.mp;
    s->host.resize((size_t)k);
    return s;
}

// What both forms of create share once s->y / s->Cb hold the columns' signs and boxes in the device's layout (`total` entries),
// `G0` the linear terms and `a0` the start in the same layout and `fold` every column's folded start: the vectors, `parts`
// partials, the cache, the start state, the start gradient (`start(S, batch, last)` launches the form's start kernel; nothing is
// launched when every folded start is zero), QD and the first selection (`first()` launches it, after QD).  `dual` is the longest
// column's dimension (libsvm's cap).  On failure s is destroyed.
template <typename START, typename FIRST>
static int mr_start(bq_mrsmo *s, const double *G0, const double *a0, const std::vector<mr_fold> &fold, size_t total, size_t parts,
                    int64_t dual, int64_t max_steps, int64_t cache_rows, START start, FIRST first, bq_mrsmo **out) {
    bq_problem *p = s->p;
    bq_ctx *c = p->ctx;
    mr_dev &P = s->P;
    const int k = P.k;
    const int64_t n = P.n;
    const size_t kN = total;
    const bool nu = s->rule == BQ_RSMO_RULE_NU;
    auto fail = [&](hipError_t e, const char *what) {
        bq_set_error("%s failed: %s", what, hipGetErrorString(e));
        hipStreamSynchronize(c->stream);
        bq_mrsmo_destroy(s);
        return e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
    };
    bq_mrsmo_cache cache = {};
    const size_t nreq_row = (size_t)(nu ? 3 : 1) * (size_t)k;
    hipError_t e = s->mem.dev(&P.alpha, kN);
    if (e == hipSuccess) e = s->mem.dev(&P.G, kN);
    if (e == hipSuccess) e = s->mem.dev(&P.y, kN);
    if (e == hipSuccess) e = s->mem.dev(&P.Cb, kN);
    if (e == hipSuccess) e = s->mem.dev(&P.QD, (size_t)n);
    if (e == hipSuccess) e = s->mem.dev(&cache.slot_of, (size_t)n);
    if (e == hipSuccess) e = s->mem.dev(&P.col, (size_t)k);
    if (e == hipSuccess) e = s->mem.dev(&P.glob, 1);
    if (e == hipSuccess) e = s->mem.dev(&P.req_row, nreq_row);
    if (e == hipSuccess) e = s->mem.dev(&P.miss_row, (size_t)MR_REQ);
    if (e == hipSuccess) e = s->mem.dev(&P.miss_slot, (size_t)MR_REQ);
    if (e == hipSuccess) e = s->mem.dev(&P.req_in, (size_t)MR_REQ);
    if (e == hipSuccess) e = s->mem.dev(&P.req_out, (size_t)MR_REQ);
    if (e == hipSuccess) e = s->mem.dev(&P.res_req, (size_t)MR_REQ);
    if (e == hipSuccess) e = s->mem.dev(&P.res_slot, (size_t)MR_REQ);
    if (e == hipSuccess) e = s->mem.dev(&P.res_pin, (size_t)MR_REQ);
    if (e == hipSuccess) e = s->mem.dev(&P.part_v, parts);
    if (e == hipSuccess) e = s->mem.dev(&P.part_k, parts);
    if (e == hipSuccess) e = s->mem.dev(&P.part_w, parts);
    if (e == hipSuccess) e = s->mem.dev(&P.part_i, parts);
    if (nu) {
        if (e == hipSuccess) e = s->mem.dev(&P.part_v2, parts);
        if (e == hipSuccess) e = s->mem.dev(&P.part_w2, parts);
        if (e == hipSuccess) e = s->mem.dev(&P.part_i2, parts);
    }
    if (e != hipSuccess) return fail(e, "the batched row-based SMO's vectors");
    // the cache: the rows asked for, or what half of the free memory holds; n rows hold every row there is
    int64_t R = cache_rows;
    if (R == 0) {
        size_t free_b = 0, total_b = 0;
        if ((e = hipMemGetInfo(&free_b, &total_b)) != hipSuccess) return fail(e, "hipMemGetInfo");
        R = std::max<int64_t>((int64_t)(free_b / 2 / (sizeof(double) * (size_t)P.pitch)), (nu ? 3 : 2) * (int64_t)k);
    }
    if (R > n) R = n;
    s->R = cache.R = R;
    if ((e = s->mem.dev(&P.cache, (size_t)R * (size_t)P.pitch)) != hipSuccess) return fail(e, "the row cache");
    if ((e = s->mem.dev(&cache.row_of, (size_t)R)) != hipSuccess) return fail(e, "the row cache");
    e = bq_dev_zeroed(e, s->mem, &cache.stamp, (size_t)R, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(cache.slot_of, 0xFF, sizeof(int) * (size_t)n, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(cache.row_of, 0xFF, sizeof(int) * (size_t)R, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(P.req_row, 0xFF, sizeof(int) * nreq_row, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(P.alpha, a0, sizeof(double) * kN, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(P.G, G0, sizeof(double) * kN, hipMemcpyHostToDevice, c->stream);   // b = 0: G0 = lin
    if (e == hipSuccess) e = hipMemcpyAsync(P.y, s->y.data(), sizeof(double) * kN, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(P.Cb, s->Cb.data(), sizeof(double) * kN, hipMemcpyHostToDevice, c->stream);
    mr_col c0 = {};
    c0.i = c0.j = c0.i2 = c0.last_i = c0.last_j = c0.slot_i = c0.slot_j = c0.slot_2 = c0.slot_u = -1;
    c0.gmax = c0.gmax2 = c0.gmaxn = c0.gmaxn2 = -INFINITY;
    std::fill(s->host.begin(), s->host.end(), c0);
    mr_glob g0 = {};
    g0.cache = cache;
    g0.cap = max_steps > 0 ? (long long)max_steps : std::max<long long>(10000000LL, 100LL * (long long)dual);   // libsvm's max_iter
    g0.cap = (long long)bq_hook_value("rsmo_max_steps", (double)g0.cap);
    g0.live = k;
    if (e == hipSuccess) e = hipMemcpyAsync(P.col, s->host.data(), sizeof(mr_col) * (size_t)k, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(P.glob, &g0, sizeof(g0), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) return fail(e, "the batched row-based SMO's start");
    // the start gradient: the ascending union of the rows with b != 0, each column's entries against it, and per batch of at most
    // min(MR_REQ, R) rows of the union each column's range of entries
    std::vector<int> uni;
    for (const mr_fold &f : fold)
        for (const auto &rb : f) uni.push_back(rb.first);
    std::sort(uni.begin(), uni.end());
    uni.erase(std::unique(uni.begin(), uni.end()), uni.end());
    const int64_t B = std::min<int64_t>(MR_REQ, R), nbatch = ((int64_t)uni.size() + B - 1) / B;
    ms_tab S = {};
    std::vector<ms_ent> ent;
    std::vector<int2> range((size_t)(nbatch * k));
    std::vector<int> has((size_t)k, 0);
    if (!uni.empty()) {
        for (int q = 0; q < k; ++q) {
            const mr_fold &f = fold[(size_t)q];
            has[(size_t)q] = f.empty() ? 0 : 1;
            const int e0 = (int)ent.size();
            for (const auto &rb : f)
                ent.push_back(ms_ent{rb.second, (int)(std::lower_bound(uni.begin(), uni.end(), rb.first) - uni.begin()), 0});
            int at = e0;   // (the entries ascend in u: one walk serves every batch)
            for (int64_t b = 0; b < nbatch; ++b) {
                const int lo = at;
                while (at < (int)ent.size() && ent[(size_t)at].u < (b + 1) * B) ++at;
                range[(size_t)(b * k + q)] = make_int2(lo, at);
            }
        }
        ms_ent *d_ent = nullptr;
        int2 *d_range = nullptr;
        int *d_has = nullptr;
        e = s->mem.dev(&d_ent, ent.size());
        if (e == hipSuccess) e = s->mem.dev(&d_range, range.size());
        if (e == hipSuccess) e = s->mem.dev(&d_has, (size_t)k);
        e = bq_dev_zeroed(e, s->mem, &S.acc, s->per ? kN : (size_t)k * (size_t)n, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_ent, ent.data(), sizeof(ms_ent) * ent.size(), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_range, range.data(), sizeof(int2) * range.size(), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_has, has.data(), sizeof(int) * (size_t)k, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return fail(e, "the start gradient's tables");
        S.ent = d_ent;
        S.range = d_range;
        S.has = d_has;
    }
    int rc = rsmo_dispatch(p, [&](auto kd) {
        for (int64_t b = 0; b < nbatch && e == hipSuccess; ++b) {   // a batch: its rows into slots (made 16 at a time), folded into every column
            const int cnt = (int)std::min<int64_t>(B, (int64_t)uni.size() - b * B);
            e = hipMemcpyAsync(P.req_in, uni.data() + b * B, sizeof(int) * (size_t)cnt, hipMemcpyHostToDevice, c->stream);
            mr_request_kernel<<<1, RSMO_T, 0, c->stream>>>(P, cnt);
            mr_launch_rows(kd, s, c->stream);
            S.u0 = (int)(b * B);
            start(S, (int)b, b == nbatch - 1 ? 1 : 0);
            mr_clear_kernel<<<1, 1, 0, c->stream>>>(P);
        }
        const unsigned int waves = (unsigned int)(P.mp / 16), per = RSMO_T / 64;
        mr_diag_kernel<decltype(kd)::kind, decltype(kd)::deg><<<(waves + per - 1) / per, RSMO_T, 0, c->stream>>>(P);
        first();
    });
    if (rc == BQ_OK && e != hipSuccess) return fail(e, "the batched row-based SMO's start gradient");
    if (rc == BQ_OK && (e = hipGetLastError()) != hipSuccess) return fail(e, "the batched row-based SMO's first selection");
    if (rc == BQ_OK) rc = mr_read_cols(s);   // (g0, c0, the tables and the caller's vectors are read by then)
    if (rc != BQ_OK) {
        hipStreamSynchronize(c->stream);
        bq_mrsmo_destroy(s);
        return rc;
    }
    s->mem.release(S.ent);   // the start's tables served the set-up only
    s->mem.release(S.range);
    s->mem.release(S.has);
    s->mem.release(S.acc);
    *out = s;
    return BQ_OK;
}

// the list form's launches 2 and 4 at the solver's positions per thread and rule (start: the start kernel of a batch)
static void ml_launch(const bq_mrsmo *s, bool select, int first, hipStream_t st, const ms_tab *start = nullptr, int batch = 0) {
    const bool nu = s->rule == BQ_RSMO_RULE_NU;
    auto go = [&](auto per) {
        constexpr int PER = decltype(per)::value;
        if (start)
            ml_start_kernel<PER><<<s->grid, RSMO_T, 0, st>>>(s->P, *start, batch, first);
        else if (select && nu)
            ml_nu_select_kernel<PER><<<s->grid, RSMO_T, 0, st>>>(s->P);
        else if (select)
            ml_select_kernel<PER><<<s->grid, RSMO_T, 0, st>>>(s->P);
        else if (nu)
            ml_nu_update_kernel<PER><<<s->grid, RSMO_T, 0, st>>>(s->P, first);
        else
            ml_update_kernel<PER><<<s->grid, RSMO_T, 0, st>>>(s->P, first);
    };
    if (s->per == 2)
        go(std::integral_constant<int, 2>());
    else if (s->per == 4)
        go(std::integral_constant<int, 4>());
    else
        go(std::integral_constant<int, ML_PER>());
}
// launches 2 and 4 of either form
static void mr_launch_step(const bq_mrsmo *s, bool select, int first, hipStream_t st) {
    if (s->per) return ml_launch(s, select, first, st);
    const dim3 grid(s->nblk, (unsigned int)s->P.k);
    const bool nu = s->rule == BQ_RSMO_RULE_NU;
    if (select && nu)
        mr_nu_select_kernel<<<grid, RSMO_T, 0, st>>>(s->P);
    else if (select)
        mr_select_kernel<<<grid, RSMO_T, 0, st>>>(s->P);
    else if (nu)
        mr_nu_update_kernel<<<grid, RSMO_T, 0, st>>>(s->P, first);
    else
        mr_update_kernel<<<grid, RSMO_T, 0, st>>>(s->P, first);
}

extern "C" int bq_mrsmo_create_general(bq_problem *p, int rule, int k, int64_t N, const double *signs, const double *lin,
                                       const double *boxes, const double *alpha0, double tol, int64_t max_steps, int64_t cache_rows,
                                       bq_mrsmo **out) {
    BQ_ARG(p && signs && lin && boxes && alpha0 && out, "NULL argument");
    BQ_TRY(mr_check(p, rule, k, tol, max_steps, cache_rows));
    const int64_t n = p->n;
    BQ_ARG(N == n || N == 2 * n, "N must be n or 2n");
    BQ_ARG(N < ((int64_t)1 << 31), "the dual dimension must stay below 2^31");
    std::vector<mr_fold> fold((size_t)k);
    for (int c = 0; c < k; ++c) {
        const double *sg = signs + (int64_t)c * N, *a0 = alpha0 + (int64_t)c * N;
        bool pos = false, neg = false;
        for (int64_t v = 0; v < N; ++v) {
            BQ_TRY(mr_check_entry(sg[v], lin[(int64_t)c * N + v], boxes[(int64_t)c * N + v], a0[v]));
            BQ_ARG(N == n || sg[v] == (v < n ? 1.0 : -1.0), "the signs of 2n variables must be [+1 ..; -1 ..]");
            pos |= sg[v] > 0.0;
            neg |= sg[v] < 0.0;
        }
        BQ_ARG(rule != BQ_RSMO_RULE_NU || (pos && neg), "Solver_NU needs both signs");
        for (int64_t t = 0; t < n; ++t) {   // b, folded to the rows
            double b = sg[t] * a0[t];
            if (N > n) b = b + sg[t + n] * a0[t + n];
            if (b != 0.0) fold[(size_t)c].push_back({(int)t, b});
        }
    }
    BQ_HIP(hipSetDevice(p->ctx->device));
    bq_mrsmo *s = mr_new(p, rule, k, tol);
    s->P.N = N;
    s->nblk = (unsigned int)((n + RSMO_T - 1) / RSMO_T);
    const size_t kN = (size_t)k * (size_t)N;
    s->y.assign(signs, signs + kN);
    s->Cb.assign(boxes, boxes + kN);
    hipStream_t st = p->ctx->stream;
    const dim3 grid(s->nblk, (unsigned int)k);
    return mr_start(s, lin, alpha0, fold, kN, (size_t)k * s->nblk, N, max_steps, cache_rows,
                    [&](const ms_tab &S, int batch, int last) { mr_start_kernel<<<grid, RSMO_T, 0, st>>>(s->P, S, batch, last); },
                    [&] { mr_launch_step(s, false, 1, st); }, out);
}

// libsvm's Solver from a zero start: the general entry with BQ_RSMO_RULE_PLAIN and alpha0 = 0 (G0 = lin, no start kernel)
extern "C" int bq_mrsmo_create(bq_problem *p, int k, int64_t N, const double *signs, const double *lin, const double *boxes, double tol,
                               int64_t max_steps, int64_t cache_rows, bq_mrsmo **out) {
    BQ_ARG(p && k >= 1 && k <= MR_REQ && N >= 1, "NULL argument, or k outside 1 .. 1024");
    const std::vector<double> zero((size_t)k * (size_t)N, 0.0);
    return bq_mrsmo_create_general(p, BQ_RSMO_RULE_PLAIN, k, N, signs, lin, boxes, zero.data(), tol, max_steps, cache_rows, out);
}

extern "C" int bq_mrsmo_create_lists_general(bq_problem *p, int rule, int k, const int64_t *offsets, const int32_t *rows,
                                             const double *signs, const double *lin, const double *boxes, const double *alpha0, double tol,
                                             int64_t max_steps, int64_t cache_rows, bq_mrsmo **out) {
    BQ_ARG(p && offsets && rows && signs && lin && boxes && alpha0 && out, "NULL argument");
    BQ_TRY(mr_check(p, rule, k, tol, max_steps, cache_rows));
    const int64_t n = p->n;
    BQ_ARG(offsets[0] == 0, "offsets must ascend from 0");
    std::vector<mr_fold> fold((size_t)k);
    for (int c = 0; c < k; ++c) {
        BQ_ARG(offsets[c + 1] > offsets[c], "every column needs at least one row: offsets must ascend strictly");
        BQ_ARG(offsets[c + 1] - offsets[c] <= n, "a list cannot be longer than the problem has rows");
        bool pos = false, neg = false;
        for (int64_t v = offsets[c]; v < offsets[c + 1]; ++v) {
            BQ_ARG(rows[v] >= 0 && rows[v] < n, "a listed row lies outside the problem");
            BQ_ARG(v == offsets[c] || rows[v] > rows[v - 1], "a column's rows must ascend strictly");
            BQ_TRY(mr_check_entry(signs[v], lin[v], boxes[v], alpha0[v]));
            pos |= signs[v] > 0.0;
            neg |= signs[v] < 0.0;
            const double b = signs[v] * alpha0[v];   // per position
            if (b != 0.0) fold[(size_t)c].push_back({(int)rows[v], b});
        }
        BQ_ARG(rule != BQ_RSMO_RULE_NU || (pos && neg), "Solver_NU needs both signs");
    }
    BQ_ARG(n < ((int64_t)1 << 31), "the dual dimension must stay below 2^31");
    int per = (int)bq_hook_value("mrsmo_list_per", (double)ML_PER);   // the slice-width comparison of profiles/ovo_smo_rows/
    if (per != 2 && per != 4) per = ML_PER;
    const int slice = RSMO_T * per;
    // the packed layout (each column at a multiple of ML_PAD; pad positions: the list's last row, +1, box 0 — never scanned) and
    // the work table: one (column, first position) per slice, column by column
    std::vector<ml_info> info((size_t)k);
    std::vector<int2> work;
    int64_t total = 0, parts = 0, longest = 0;
    for (int c = 0; c < k; ++c) {
        const int64_t m = offsets[c + 1] - offsets[c], nsl = (m + slice - 1) / slice;
        info[(size_t)c] = ml_info{total, (int)m, (int)nsl, (int)parts, 0};
        for (int64_t b = 0; b < nsl; ++b) work.push_back(make_int2(c, (int)(b * slice)));
        total += (m + ML_PAD - 1) / ML_PAD * ML_PAD;
        parts += nsl;
        longest = std::max(longest, m);
    }
    BQ_ARG(parts < ((int64_t)1 << 31) && total < ((int64_t)1 << 40), "the lists are too long for one solver");
    std::vector<double> G0((size_t)total, 0.0), a0((size_t)total, 0.0);
    std::vector<int> list((size_t)total, 0);
    BQ_HIP(hipSetDevice(p->ctx->device));
    bq_mrsmo *s = mr_new(p, rule, k, tol);
    s->P.N = 0;
    s->per = per;
    s->grid = (unsigned int)parts;
    s->y.assign((size_t)total, 1.0);
    s->Cb.assign((size_t)total, 0.0);
    for (int c = 0; c < k; ++c) {
        const ml_info &in = info[(size_t)c];
        const int64_t src = offsets[c], mpad = (in.m + ML_PAD - 1) / ML_PAD * ML_PAD;
        for (int64_t q = 0; q < mpad; ++q) {
            const bool live = q < in.m;
            list[(size_t)(in.off + q)] = rows[src + (live ? q : in.m - 1)];
            if (!live) continue;
            s->y[(size_t)(in.off + q)] = signs[src + q];
            s->Cb[(size_t)(in.off + q)] = boxes[src + q];
            G0[(size_t)(in.off + q)] = lin[src + q];
            a0[(size_t)(in.off + q)] = alpha0[src + q];
        }
    }
    s->info = info;
    // the tables go up before mr_start's own uploads; mr_start synchronises the stream before it returns, on every path
    bq_ctx *c = p->ctx;
    int *d_rows = nullptr;
    ml_info *d_info = nullptr;
    int2 *d_work = nullptr;
    hipError_t e = s->mem.dev(&d_rows, (size_t)total);
    if (e == hipSuccess) e = s->mem.dev(&d_info, (size_t)k);
    if (e == hipSuccess) e = s->mem.dev(&d_work, work.size());
    if (e == hipSuccess) e = hipMemcpyAsync(d_rows, list.data(), sizeof(int) * (size_t)total, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_info, info.data(), sizeof(ml_info) * (size_t)k, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_work, work.data(), sizeof(int2) * work.size(), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) {
        bq_set_error("the row lists failed: %s", hipGetErrorString(e));
        hipStreamSynchronize(c->stream);
        bq_mrsmo_destroy(s);
        return e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
    }
    s->P.rows = d_rows;
    s->P.info = d_info;
    s->P.work = d_work;
    return mr_start(s, G0.data(), a0.data(), fold, (size_t)total, (size_t)parts, longest, max_steps, cache_rows,
                    [&](const ms_tab &S, int batch, int last) { ml_launch(s, false, last, c->stream, &S, batch); },
                    [&] { ml_launch(s, false, 1, c->stream); }, out);
}

extern "C" int bq_mrsmo_create_lists(bq_problem *p, int k, const int64_t *offsets, const int32_t *rows, const double *signs,
                                     const double *lin, const double *boxes, double tol, int64_t max_steps, int64_t cache_rows,
                                     bq_mrsmo **out) {
    BQ_ARG(p && offsets && k >= 1 && k <= MR_REQ, "NULL argument, or k outside 1 .. 1024");
    BQ_ARG(offsets[0] == 0 && offsets[k] >= 0, "offsets must ascend from 0");
    const std::vector<double> zero((size_t)offsets[k], 0.0);
    return bq_mrsmo_create_lists_general(p, BQ_RSMO_RULE_PLAIN, k, offsets, rows, signs, lin, boxes, zero.data(), tol, max_steps,
                                         cache_rows, out);
}

extern "C" int bq_mrsmo_run(bq_mrsmo *s, int64_t max_steps, int64_t *steps, int *finished) {
    BQ_ARG(s && steps && finished, "NULL argument");
    BQ_ARG(max_steps > 0, "max_steps must be > 0");
    bq_ctx *c = s->p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    if (!s->done) {
        BQ_TRY(rsmo_dispatch(s->p, [&](auto kd) {
            for (int64_t q = 0; q < max_steps; ++q) {
                mr_launch_rows(kd, s, c->stream);
                mr_launch_step(s, true, 0, c->stream);
                mr_launch_rows(kd, s, c->stream);
                mr_launch_step(s, false, 0, c->stream);
            }
        }));
        BQ_HIP(hipGetLastError());
        BQ_TRY(mr_read_cols(s));
    }
    for (int q = 0; q < s->P.k; ++q) {
        steps[q] = s->host[(size_t)q].steps;
        finished[q] = s->host[(size_t)q].finished;
    }
    return BQ_OK;
}

extern "C" int bq_mrsmo_get(bq_mrsmo *s, int what, int column, double *out) {
    BQ_ARG(s && out, "NULL argument");
    BQ_ARG(what >= BQ_RSMO_ALPHAS && what <= BQ_RSMO_NU_SCALARS, "what");
    BQ_ARG(what != BQ_RSMO_NU_SCALARS || s->rule == BQ_RSMO_RULE_NU, "BQ_RSMO_NU_SCALARS needs a BQ_RSMO_RULE_NU solver");
    BQ_ARG(what == BQ_RSMO_STATS || (column >= 0 && column < s->P.k), "column");
    bq_ctx *c = s->p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    const mr_dev &P = s->P;
    // a column's entries and where they start: c N in the full-column form, the packed offset of its list in the list form
    const bool stats = what == BQ_RSMO_STATS;
    const size_t N = stats || !s->per ? (size_t)P.N : (size_t)s->info[(size_t)column].m;
    const size_t off = stats ? 0 : s->per ? (size_t)s->info[(size_t)column].off : (size_t)column * N;
    if (what == BQ_RSMO_ALPHAS || what == BQ_RSMO_GRADIENT) {
        BQ_HIP(hipMemcpyAsync(out, (what == BQ_RSMO_ALPHAS ? P.alpha : P.G) + off, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
        BQ_HIP(hipStreamSynchronize(c->stream));
        return BQ_OK;
    }
    if (what == BQ_RSMO_STATS) {
        mr_glob g;
        BQ_HIP(hipMemcpyAsync(&g, P.glob, sizeof(g), hipMemcpyDeviceToHost, c->stream));
        BQ_HIP(hipStreamSynchronize(c->stream));
        out[0] = (double)g.cache.hits;
        out[1] = (double)g.cache.misses;
        out[2] = (double)s->R;
        return BQ_OK;
    }
    // calculate_rho in libsvm's order, on the host
    std::vector<double> a(N), g(N);
    BQ_HIP(hipMemcpyAsync(a.data(), P.alpha + off, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
    BQ_HIP(hipMemcpyAsync(g.data(), P.G + off, sizeof(double) * N, hipMemcpyDeviceToHost, c->stream));
    BQ_TRY(mr_read_cols(s));
    const mr_col &cc = s->host[(size_t)column];
    if (s->rule == BQ_RSMO_RULE_NU) {   // Solver_NU::calculate_rho; BQ_RSMO_SCALARS: the same rho, then the positive side's maxima
        bq_rsmo_nu_rho nu;
        for (size_t t = 0; t < N; ++t) bq_rsmo_nu_rho_add(&nu, s->y[off + t], a[t], s->Cb[off + t], g[t]);
        double r = 0.0;
        bq_rsmo_nu_rho_value(&nu, &out[0], &r);
        if (what == BQ_RSMO_NU_SCALARS) {
            out[1] = r;
            out[2] = bq_rsmo_nu_gap(cc.gmax, cc.gmax2);
            out[3] = bq_rsmo_nu_gap(cc.gmaxn, cc.gmaxn2);
            out[4] = (double)cc.last_i;
            out[5] = (double)cc.last_j;
            out[6] = (double)cc.steps;
            return BQ_OK;
        }
    } else {
        bq_rsmo_rho rho;
        for (size_t t = 0; t < N; ++t) bq_rsmo_rho_add(&rho, s->y[off + t], a[t], s->Cb[off + t], g[t]);
        out[0] = bq_rsmo_rho_value(&rho);
    }
    out[1] = cc.gmax;
    out[2] = cc.gmax2;
    out[3] = (double)cc.last_i;
    out[4] = (double)cc.last_j;
    out[5] = (double)cc.steps;
    return BQ_OK;
}

extern "C" int bq_mrsmo_rows(bq_mrsmo *s, int m, const int64_t *idx, double *out) {
    BQ_ARG(s && idx && out, "NULL argument");
    BQ_ARG(m >= 1, "m must be >= 1");
    const mr_dev &P = s->P;
    for (int q = 0; q < m; ++q) BQ_ARG(idx[q] >= 0 && idx[q] < P.n, "a requested row lies outside the problem");
    bq_ctx *c = s->p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    // a call resolves what fits beside the rows the live columns wait for
    const int batch = (int)std::min<int64_t>(MR_REQ, std::max<int64_t>(1, s->R - (int64_t)P.nreq * P.k));
    std::vector<int> rows((size_t)batch), slots((size_t)batch);
    int rc = BQ_OK;
    for (int q0 = 0; q0 < m && rc == BQ_OK; q0 += batch) {
        const int cnt = std::min(batch, m - q0);
        for (int q = 0; q < cnt; ++q) rows[(size_t)q] = (int)idx[q0 + q];
        BQ_HIP(hipMemcpyAsync(P.req_in, rows.data(), sizeof(int) * (size_t)cnt, hipMemcpyHostToDevice, c->stream));
        rc = rsmo_dispatch(s->p, [&](auto kd) {
            mr_launch_rows(kd, s, c->stream);   // the rows the step in hand still waits for
            mr_request_kernel<<<1, RSMO_T, 0, c->stream>>>(P, cnt);
            mr_launch_rows(kd, s, c->stream);
            mr_clear_kernel<<<1, 1, 0, c->stream>>>(P);
        });
        BQ_HIP(hipGetLastError());
        BQ_HIP(hipMemcpyAsync(slots.data(), P.req_out, sizeof(int) * (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
        BQ_HIP(hipStreamSynchronize(c->stream));
        for (int q = 0; q < cnt; ++q) {
            if (slots[(size_t)q] < 0) {
                bq_set_error("the row cache has no free slot beside the rows of the step in hand");
                return BQ_ERR_BADARG;
            }
            BQ_HIP(hipMemcpyAsync(out + (size_t)(q0 + q) * (size_t)P.n, P.cache + (size_t)slots[(size_t)q] * (size_t)P.pitch,
                                  sizeof(double) * (size_t)P.n, hipMemcpyDeviceToHost, c->stream));
        }
        BQ_HIP(hipStreamSynchronize(c->stream));   // the slots may be evicted by the next batch
    }
    return rc;
}
