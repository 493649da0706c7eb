// Decision values of k estimators in ONE pass over the kernel values:
//
//   OUT[c][i] = sum_j W[c][j] * kernel(SV[j], Xt[i]) + b[c]          c < k, i < t, j < m
//
// Every 128 x 128 tile of kernel(SV, Xt) is formed once on the fp64 matrix cores (bq_mfma_tile_128, A = the SV image, B = the
// image of the test points), mapped in the accumulator registers (the maps of gram_mfma_kernel's epilogue, statement for
// statement) and contracted with the coefficient columns by a SECOND set of v_mfma_f64_16x16x4_f64 without leaving the
// registers: nothing of size t x m exists in memory, and no kernel value passes through LDS.
//
// The contraction.  A tile is computed as SV rows x test columns, so register v of accumulator acc[i][j] of a lane holds the
// kernel value of SV row bq_acc_row(i, v) — MFMA row (lane >> 4) + 4 v of row block i — and test point lane & 15 of column
// block j.  Read as the A operand of another 16x16x4 MFMA (row = lane & 15, k = lane >> 4) that register is the 16 test points
// x 4 SV rows {4 v .. 4 v + 3} slice of the block; the matching B operand (k = lane >> 4, column = lane & 15) is
// W[column][that SV row], one load per lane from the SV-major coefficient image Wt[mp][kp].  The 16 (i, v) of a wave add
// their slices, in that order, to out[j][g]: 16 test points x 16 columns of group g, C/D layout column = lane & 15, test
// point = (lane >> 4) + 4 reg of column block j.  64 MFMAs per wave, tile and group of 16 columns, against 16 (d / 4) for the
// dot products.
//
// Columns.  The output accumulators (32 VGPRs per group and lane) stay live across the workgroup's whole walk over SV tiles.
// With one group the kernel keeps the Gram build's two workgroups per CU, whose epilogues hide behind each other's MFMAs;
// more than 16 columns take the GMAX = 4 instantiation, which holds up to four groups (64 columns, 128 VGPRs) at one
// workgroup per CU and skips the groups it does not have.  Beyond 64 columns further passes (blockIdx.z) form the kernel
// values again.  A column's sum does not depend on its group, its slot or the instantiation: an MFMA forms each output
// column from that column of B alone, and both instantiations are one source.
//
// Order of every sum (no atomics): within a wave over (i, v); then wave row 0 + wave row 1 (LDS); then the SV tiles of a
// unit in ascending order in the registers; then the units in ascending order (decide_reduce_kernel).  The SV range is cut
// into units of U tiles so that few test points still fill the chip; U depends on (t, m, d) only.
#include "bq_common.h"
#include "bq_scratch.h"

#include "bq_gram_image.h"
#include "bq_mfma_tile.h"

#include <algorithm>
#include <vector>

struct decide_params {
    const double *At, *Bt;   // k-major padded images: SV At[dp][mp], test points Bt[dp][tp]
    const double *a2, *b2;   // their squared row norms (padded)
    const double *Wt;        // coefficients, SV-major: Wt[mp][kp], zero beyond m and k
    double *part;            // per-unit partial sums: part[unit][test row of the chunk][kp]
    int64_t mp, tp, dp, kp;
    int64_t tile0;           // first test tile of this launch's chunk
    int64_t rows;            // padded test rows of a chunk (pitch of a unit in part)
    int tiles_m, U;          // SV tiles, SV tiles per unit
    int groups;              // groups of 16 columns = kp / 16
    int degree;
    double gamma, coef0;
};

// DEG: the polynomial kernel's degree when it is 1, 2 or 3, else 0 (pow).  A template argument, not a branch around three epilogues
// as in gram_mfma_kernel: with the output accumulators live across it the joined paths spilled (68 VGPRs at GMAX = 1).
template <int KIND, int GMAX, int DEG>
__global__ __launch_bounds__(256, GMAX == 1 ? 2 : 1) void decide_multi_kernel(decide_params P) {
    __shared__ __attribute__((aligned(16))) bq_tile_smem sm;
    __shared__ double rowsq[4][64];   // squared norms of each wave's 64 SV rows, per tile (through LDS as in gram_mfma_kernel)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wr = wv >> 1, wc = wv & 1, ccol = lane & 15, crow = lane >> 4;
    const int64_t bcol = (P.tile0 + blockIdx.x) * BQ_GT;   // this workgroup's 128 test points
    const int unit = blockIdx.y, g0 = blockIdx.z * GMAX;
    const int ng = P.groups - g0 < GMAX ? P.groups - g0 : GMAX;
    const int i0 = unit * P.U, i1 = i0 + P.U < P.tiles_m ? i0 + P.U : P.tiles_m;
    bq_d4 out[4][GMAX];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int g = 0; g < GMAX; ++g) out[j][g] = (bq_d4){0.0, 0.0, 0.0, 0.0};
    for (int I = i0; I < i1; ++I) {
        const int64_t arow = (int64_t)I * BQ_GT;
        if (KIND == BQ_KERNEL_RBF) rowsq[wv][lane] = P.a2[arow + wr * 64 + lane];
        bq_d4 acc[4][4];
        bq_tile_zero(acc);
        bq_mfma_tile_128(P.At, P.mp, arow, P.Bt, P.tp, bcol, P.dp, sm, acc);
        // as in gram_mfma_kernel: what the epilogue reads must not be hoisted over the MFMA loop
        int64_t opaque = 0;
        asm volatile("" : "+s"(opaque));
        double bj[4];   // the squared norms of this lane's four test points
#pragma unroll
        for (int j = 0; j < 4; ++j) bj[j] = KIND == BQ_KERNEL_RBF ? P.b2[opaque + bcol + bq_acc_col(2 * (j >> 1)) + (j & 1)] : 0.0;
        // this lane's coefficient of SV row bq_acc_row(i, v) and column 16 (g0 + g) + ccol: sixteen lanes read 128 contiguous bytes
        const double *const wlane = P.Wt + (opaque + arow + wr * 64 + 2 * crow) * P.kp + g0 * 16 + ccol;
        {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double wf[4][GMAX];
#pragma unroll
                for (int v = 0; v < 4; ++v)
#pragma unroll
                    for (int g = 0; g < GMAX; ++g)
                        wf[v][g] = g < ng ? wlane[(int64_t)((i >> 1) * 32 + 8 * v + (i & 1)) * P.kp + g * 16] : 0.0;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const double ai = KIND == BQ_KERNEL_RBF ? rowsq[wv][bq_acc_row64(i, v)] : 0.0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double dot = acc[i][j][v];
                        double kv;
                        if (KIND == BQ_KERNEL_RBF) {
                            double dist = -2.0 * dot;
                            dist += ai;
                            dist += bj[j];
                            dist = fmax(dist, 0.0);
                            kv = bq_exp(-P.gamma * dist);
                        } else if (KIND == BQ_KERNEL_POLY) {
                            kv = bq_poly_map<DEG>(P.gamma * dot + P.coef0, P.degree);
                        } else if (KIND == BQ_KERNEL_SIGMOID) {
                            kv = tanh(P.gamma * dot + P.coef0);
                        } else {
                            kv = dot;
                        }
                        acc[i][j][v] = kv;
                    }
                    if (KIND == BQ_KERNEL_RBF || KIND == BQ_KERNEL_POLY) __builtin_amdgcn_sched_barrier(0);   // four chains in flight
                }
#pragma unroll
                for (int v = 0; v < 4; ++v)
#pragma unroll
                    for (int g = 0; g < GMAX; ++g)
                        if (g < ng) {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                out[j][g] = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[i][j][v], wf[v][g], out[j][g], 0, 0, 0);
                        }
            }
        }
        __syncthreads();   // the next tile's prologue refills the LDS buffers (and, after the last tile, the meeting below)
    }
    // the two wave rows hold sums over different SV rows of the same test points: row 1 hands its sums over through the tile
    // buffers (exactly their 64 KiB at GMAX = 4), row 0 adds them to its own and stores the unit's partial sums
    bq_d4 *const red = reinterpret_cast<bq_d4 *>(&sm);
    static_assert(sizeof(bq_tile_smem) >= sizeof(bq_d4) * 2 * GMAX * 4 * 64, "the meeting buffer is the tile buffers");
    if (wr == 1) {
#pragma unroll
        for (int g = 0; g < GMAX; ++g)
#pragma unroll
            for (int j = 0; j < 4; ++j) red[((wc * GMAX + g) * 4 + j) * 64 + lane] = out[j][g];
    }
    __syncthreads();
    if (wr == 0) {
        double *const prow = P.part + ((int64_t)unit * P.rows + (int64_t)blockIdx.x * BQ_GT + wc * 64) * P.kp + g0 * 16 + ccol;
#pragma unroll
        for (int g = 0; g < GMAX; ++g)
            if (g < ng) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bq_d4 o = out[j][g] + red[((wc * GMAX + g) * 4 + j) * 64 + lane];
#pragma unroll
                    for (int r = 0; r < 4; ++r)   // test point (crow + 4 r) of column block j, as bq_acc_col64 numbers it
                        prow[(int64_t)((j >> 1) * 32 + 2 * (crow + 4 * r) + (j & 1)) * P.kp + g * 16] = o[r];
                }
            }
    }
}

// out[c][r0 + i] = (the units' partial sums of (i, c), in unit order) + b[c]
__global__ __launch_bounds__(256) void decide_reduce_kernel(const double *__restrict__ part, int units, int64_t rows, int64_t kp,
                                                            int64_t nrows, int k, const double *__restrict__ b,
                                                            double *__restrict__ out, int64_t t, int64_t r0) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nrows * k) return;
    const int64_t i = idx / k;
    const int c = (int)(idx % k);
    double s = part[i * kp + c];
    for (int u = 1; u < units; ++u) s += part[((int64_t)u * rows + i) * kp + c];
    out[(int64_t)c * t + r0 + i] = s + b[c];
}

// SV tiles per unit: enough workgroups for two per CU of a 256-CU part whenever the SV range allows it.  A function of
// (t, m, d) only — the association of every sum is fixed by the problem's shape (hook decision_multi_unit forces it in tests).
static int64_t decide_unit_tiles(int64_t t, int64_t m, int64_t d) {
    (void)d;
    const int64_t tiles_t = (t + BQ_GT - 1) / BQ_GT, tiles_m = (m + BQ_GT - 1) / BQ_GT;
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(tiles_m, (512 + tiles_t - 1) / tiles_t));
    return (tiles_m + want - 1) / want;
}

int bq_launch_decision_multi(bq_ctx *ctx, int kernel, double gamma, double coef0, int degree, int64_t m, int64_t d,
                             const double *SV, int k, const double *W, const double *b, int64_t t, const double *Xt,
                             double *out, bq_decision_chunk_fn after_chunk, void *arg) {
    bq_scratch mem;   // declared first: freed after every path's last use of the stream
    gram_images A, B;
    const int64_t kp = bq_round_up(k, 16), mp = bq_round_up(m, BQ_GT), tp = bq_round_up(t, BQ_GT);
    const int64_t tiles_m = mp / BQ_GT;
    int64_t U = decide_unit_tiles(t, m, d);
    {
        double hv = 0.0;
        if (bq_hook("decision_multi_unit", &hv) && hv >= 1.0) U = std::min<int64_t>((int64_t)hv, tiles_m);
    }
    const int64_t units = (tiles_m + U - 1) / U;
    // test points per launch: the partial sums of a chunk take <= 256 MiB.  Every output row is formed by the same workgroup
    // program on the same operands whatever the chunk: the values do not depend on it (hook decision_multi_chunk_rows)
    int64_t chunk = std::max<int64_t>(BQ_GT, ((int64_t)1 << 25) / (units * kp) / BQ_GT * BQ_GT);
    {
        double hv = 0.0;
        if (bq_hook("decision_multi_chunk_rows", &hv) && hv >= 1.0) chunk = bq_round_up((int64_t)hv, BQ_GT);
    }
    chunk = std::min(chunk, tp);
    BQ_ARG(units <= 65535 && chunk / BQ_GT <= 2147483647, "decision grid too large");
    const int gmax = kp <= 16 ? 1 : 4;
    const int64_t groups = kp / 16, passes = (groups + gmax - 1) / gmax;
    auto cleanup = [&]() {   // every return past this point: nothing of this frame (hW, hb, the images, mem) is in flight afterwards
        (void)hipStreamSynchronize(ctx->stream);
    };
#define DEC_HIP(e)                                                          \
    do {                                                                    \
        hipError_t _e = (e);                                                \
        if (_e != hipSuccess) {                                             \
            bq_set_error("%s failed: %s", #e, hipGetErrorString(_e));       \
            cleanup();                                                      \
            return BQ_ERR_HIP;                                              \
        }                                                                   \
    } while (0)
    // the coefficient image: SV-major, one 16-column group contiguous per SV row, zero on the padding (a padded SV row's kernel
    // value is finite and meets a zero)
    std::vector<double> hW((size_t)(mp * kp), 0.0), hb((size_t)kp, 0.0);
    for (int c = 0; c < k; ++c) {
        const double *wc = W + (int64_t)c * m;
        for (int64_t j = 0; j < m; ++j) hW[(size_t)(j * kp + c)] = wc[j];
        if (b) hb[(size_t)c] = b[c];
    }
    double *dSV = mem.dev<double>(m * d), *dXt = mem.dev<double>(t * d), *dW = mem.dev<double>(mp * kp), *db = mem.dev<double>(kp);
    double *part = mem.dev<double>(units * chunk * kp), *dout = mem.dev<double>((int64_t)k * t);
    DEC_HIP(mem.error());
    DEC_HIP(hipMemcpyAsync(dSV, SV, sizeof(double) * m * d, hipMemcpyHostToDevice, ctx->stream));
    DEC_HIP(hipMemcpyAsync(dXt, Xt, sizeof(double) * t * d, hipMemcpyHostToDevice, ctx->stream));
    DEC_HIP(hipMemcpyAsync(dW, hW.data(), sizeof(double) * mp * kp, hipMemcpyHostToDevice, ctx->stream));
    DEC_HIP(hipMemcpyAsync(db, hb.data(), sizeof(double) * kp, hipMemcpyHostToDevice, ctx->stream));
    int rc = BQ_OK;
    if ((rc = make_image(ctx, dSV, m, d, &A)) != BQ_OK || (rc = make_image(ctx, dXt, t, d, &B)) != BQ_OK) {
        cleanup();
        return rc;
    }
    decide_params P;
    P.At = A.At;
    P.Bt = B.At;
    P.a2 = A.a2;
    P.b2 = B.a2;
    P.Wt = dW;
    P.part = part;
    P.mp = A.mp;
    P.tp = B.mp;
    P.dp = A.dp;
    P.kp = kp;
    P.rows = chunk;
    P.tiles_m = (int)tiles_m;
    P.U = (int)U;
    P.groups = (int)groups;
    P.degree = degree;
    P.gamma = gamma;
    P.coef0 = coef0;
    for (int64_t r0 = 0; r0 < t; r0 += chunk) {
        const int64_t r1 = std::min(t, r0 + chunk);
        P.tile0 = r0 / BQ_GT;
        const dim3 grid((unsigned)((r1 - r0 + BQ_GT - 1) / BQ_GT), (unsigned)units, (unsigned)passes);
#define BQ_DECIDE_LAUNCH(KIND, DEG)                                                  \
    do {                                                                             \
        if (gmax == 1)                                                               \
            decide_multi_kernel<KIND, 1, DEG><<<grid, 256, 0, ctx->stream>>>(P);    \
        else                                                                         \
            decide_multi_kernel<KIND, 4, DEG><<<grid, 256, 0, ctx->stream>>>(P);    \
    } while (0)
        switch (kernel) {
            case BQ_KERNEL_RBF: BQ_DECIDE_LAUNCH(BQ_KERNEL_RBF, 0); break;
            case BQ_KERNEL_POLY:
                if (degree == 3)
                    BQ_DECIDE_LAUNCH(BQ_KERNEL_POLY, 3);
                else if (degree == 2)
                    BQ_DECIDE_LAUNCH(BQ_KERNEL_POLY, 2);
                else if (degree == 1)
                    BQ_DECIDE_LAUNCH(BQ_KERNEL_POLY, 1);
                else
                    BQ_DECIDE_LAUNCH(BQ_KERNEL_POLY, 0);
                break;
            case BQ_KERNEL_SIGMOID: BQ_DECIDE_LAUNCH(BQ_KERNEL_SIGMOID, 0); break;
            default: BQ_DECIDE_LAUNCH(BQ_KERNEL_LINEAR, 0); break;
        }
#undef BQ_DECIDE_LAUNCH
        DEC_HIP(hipGetLastError());
        const int64_t cells = (r1 - r0) * k;
        decide_reduce_kernel<<<(unsigned)((cells + 255) / 256), 256, 0, ctx->stream>>>(part, (int)units, chunk, kp, r1 - r0, k, db,
                                                                                      dout, t, r0);
        DEC_HIP(hipGetLastError());
        if (after_chunk && (rc = after_chunk(arg, dout, r0, r1)) != BQ_OK) {
            cleanup();
            return rc;
        }
    }
    if (out) DEC_HIP(hipMemcpyAsync(out, dout, sizeof(double) * (int64_t)k * t, hipMemcpyDeviceToHost, ctx->stream));
    DEC_HIP(hipStreamSynchronize(ctx->stream));
    cleanup();
#undef DEC_HIP
    return BQ_OK;
}
