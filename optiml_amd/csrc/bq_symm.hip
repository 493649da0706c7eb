// Multi-column symmetric panel product: OUT[:, s] = P W[:, s] (P = K or K + 1, the packed lower-triangle panel of bq_symv.hip) for
// the slots s < *nlive of W, streaming the panel ONCE per chunk of SCK columns.  The one-vs-rest SVC duals of k classes share one
// Gram panel (Q_c x = y_c o ((K + 1)(y_c o x))): with k columns per stream, every panel element loaded does 2 SCK fma instead of 2.
//
// Blocking (VALU): a STRIP is SJG = 2 consecutive tiles of one tile row (2 x 2 KiB contiguous per row); a workgroup of four waves
// streams its 256 rows, SSR = 2 rows per step per wave, all SJG x SSR rows of a step in flight before the first use.  Per column a
// lane keeps the same state as the one-column kernel keeps for its one column: the direction of its 4 columns of every strip tile
// (wj0 / wj1) and their column sums (ca), so registers grow with SCK x SJG — SJG = 8 (the one-column kernel's strip) and SCK = 4
// would be 384 VGPRs; SJG = 2 x SCK = 4 with SSR = 2 is what fits without spilling (kernel-resource-usage: no scratch).  The SCK x SSR
// = 8 row partials of a step go through the one-column kernel's eight-value halving butterfly.  Slab: per column, one entry per
// off-diagonal tile plus one row part per strip, i.e. 2 KiB x (nb^2/2 + nb^2/(2 SJG)) each way (~1.2 % of the fp64 panel bytes per
// column round trip); the slab holds one chunk (SCK columns), the chunks run one after another.
// (Not built: fp64 MFMA (v_mfma_f64_16x16x4_f64) on K_IJ W_J and K_IJ' W_I with W padded to 16 columns.  At SCK = 4 the VALU work is
// 8 fma per 8-byte element, about a third of the chip's fp64 VALU rate at 8 TB/s, so this product is bound by the panel stream and
// by its slab traffic, not by arithmetic; MFMA would pay for columns only past ~16 per stream.)
//
// Determinism and batch invariance: column s's value is a function of W[:, s] alone — its arithmetic (fma chains over the strip in
// column order, the butterfly's lane tree, the four-wave column sum, the slab walk of seg_thread_sum with one segment) is the same
// for every slot and every chunk, and no atomics are used.  So a class gives the same bits alone, in any batch and at any position.
// It is NOT bit-identical to the one-column kernel (its association is tied to JG = 8 and to the canonical segments); it agrees with
// it to rounding.
//
// This file's own part is the 4-column VALU strip kernel; its association is its own, so it shares no body with the other product
// kernels.  Shared: the storage dispatch of bq_launch_symm (bq_panel_dispatch, bq_c7.h), the slab walk (slab_walk under
// seg_thread_sum, bq_symv_tile.h) and the one-off host product around the launcher (bq_product_once, below).
#include "bq_common.h"
#include "bq_scratch.h"
#include "bq_symv_tile.h"

constexpr int SJG = 2;   // tiles per strip
constexpr int SSR = 2;   // rows per step and wave
static_assert(BQ_SYMM_CK * SSR == 8, "the row partials of a step are the eight values of the halving butterfly");

template <typename T, bool ADD_ONE>
__global__ __launch_bounds__(256, 2) void symm_tiles_kernel(bq_pptr<T> panel, int64_t nb, const double *__restrict__ W,
                                                          int64_t ldw, double *__restrict__ slab, const int *__restrict__ nlive, int ch) {
    constexpr int CK = BQ_SYMM_CK;
    if (ch * CK >= *nlive) return;
    __shared__ double colred[4][ST];
    const int64_t t = (int64_t)blockIdx.x;
    int64_t I = (int64_t)sqrt(2.0 * (double)SJG * (double)t);
    if (I >= nb) I = nb - 1;
    while (I > 0 && strips_before<SJG>(I) > t) --I;
    while (strips_before<SJG>(I + 1) <= t) ++I;
    const int64_t J0 = (t - strips_before<SJG>(I)) * SJG;
    const int nj = (int)((J0 + SJG <= I + 1) ? SJG : (I + 1 - J0));

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // packed layout (bq_sym_addr): SJG tiles from a multiple of SJG lie inside ONE strip of the layout, whose pitch their rows have
    static_assert(BQ_SYM_STRIP % SJG == 0, "a strip of this kernel lies inside one strip of the layout");
    const int64_t gl = J0 / BQ_SYM_STRIP, pitch = bq_sym_strip_w(I, gl);
    const auto rows = panel + (bq_sym_strip_off(I, gl) + (int64_t)(__builtin_amdgcn_readfirstlane(wv) * 64) * pitch + (J0 - gl * BQ_SYM_STRIP) * ST);
    const double *Wc = W + (int64_t)ch * CK * ldw;
    const int c0 = tile_ld<T>::c0(lane), c1 = tile_ld<T>::c1(lane);
    d2_t wj0[CK][SJG], wj1[CK][SJG];
    double ca[CK][SJG][4];
#pragma unroll
    for (int c = 0; c < CK; ++c) {
#pragma unroll
        for (int j = 0; j < SJG; ++j) {
            const double *wJ = Wc + c * ldw + (J0 + (j < nj ? j : 0)) * ST;
            wj0[c][j] = *reinterpret_cast<const d2_t *>(wJ + c0);
            wj1[c][j] = *reinterpret_cast<const d2_t *>(wJ + c1);
            ca[c][j][0] = ca[c][j][1] = ca[c][j][2] = ca[c][j][3] = 0.0;
        }
    }
    const int64_t cs = nb * nb * ST;   // slab stride of one column
    double *rowout = slab + (I * nb + J0) * ST + wv * 64;
    const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;

#pragma unroll 1
    for (int step = 0; step < 64 / SSR; ++step) {
        d2_t a[SJG][SSR], b[SJG][SSR];
#pragma unroll
        for (int j = 0; j < SJG; ++j) {
#pragma unroll
            for (int k = 0; k < SSR; ++k) {
                if (j < nj) {
                    tile_ld<T>::get(rows + (int64_t)(step * SSR + k) * pitch + j * ST, lane, a[j][k], b[j][k]);
                } else {
                    a[j][k] = (d2_t){0.0, 0.0};
                    b[j][k] = (d2_t){0.0, 0.0};
                }
            }
        }
        double rp[CK * SSR], wi[CK][SSR];
#pragma unroll
        for (int c = 0; c < CK; ++c) {
#pragma unroll
            for (int k = 0; k < SSR; ++k) {
                rp[c * SSR + k] = 0.0;
                wi[c][k] = Wc[c * ldw + I * ST + wv * 64 + step * SSR + k];
            }
        }
#pragma unroll
        for (int j = 0; j < SJG; ++j) {
            if (j < nj) {
#pragma unroll
                for (int k = 0; k < SSR; ++k) {
                    d2_t x = a[j][k], y = b[j][k];
                    if (ADD_ONE) {
                        x.x += 1.0;
                        x.y += 1.0;
                        y.x += 1.0;
                        y.y += 1.0;
                    }
#pragma unroll
                    for (int c = 0; c < CK; ++c) {
                        double &r = rp[c * SSR + k];
                        r = fma(y.y, wj1[c][j].y, fma(y.x, wj1[c][j].x, fma(x.y, wj0[c][j].y, fma(x.x, wj0[c][j].x, r))));
                        ca[c][j][0] = fma(x.x, wi[c][k], ca[c][j][0]);
                        ca[c][j][1] = fma(x.y, wi[c][k], ca[c][j][1]);
                        ca[c][j][2] = fma(y.x, wi[c][k], ca[c][j][2]);
                        ca[c][j][3] = fma(y.y, wi[c][k], ca[c][j][3]);
                    }
                }
            }
        }
        // halving butterfly (bq_symv.hip, SR = 8): eight row partials x 64 lanes -> value rho = c * SSR + k in each 8-lane group
        double u[4], t2[2], s1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double send = b5 ? rp[i] : rp[i + 4];
            const double keep = b5 ? rp[i + 4] : rp[i];
            u[i] = keep + __shfl_xor(send, 32, 64);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const double send = b4 ? u[i] : u[i + 2];
            const double keep = b4 ? u[i + 2] : u[i];
            t2[i] = keep + __shfl_xor(send, 16, 64);
        }
        {
            const double send = b3 ? t2[0] : t2[1];
            const double keep = b3 ? t2[1] : t2[0];
            s1 = keep + __shfl_xor(send, 8, 64);
        }
        s1 += __shfl_xor(s1, 4, 64);
        s1 += __shfl_xor(s1, 2, 64);
        s1 += __shfl_xor(s1, 1, 64);
        const int rho = (b5 ? 4 : 0) + (b4 ? 2 : 0) + (b3 ? 1 : 0);
        if ((lane & 7) == 0) rowout[(rho / SSR) * cs + step * SSR + rho % SSR] = s1;
    }
    // column parts of every off-diagonal tile of the strip, one column after another
#pragma unroll
    for (int j = 0; j < SJG; ++j) {
        if (j < nj && J0 + j != I) {   // uniform across the workgroup
#pragma unroll
            for (int c = 0; c < CK; ++c) {
                __syncthreads();
                colred[wv][c0] = ca[c][j][0];
                colred[wv][c0 + 1] = ca[c][j][1];
                colred[wv][c1] = ca[c][j][2];
                colred[wv][c1 + 1] = ca[c][j][3];
                __syncthreads();
                slab[c * cs + ((J0 + j) * nb + I) * ST + tid] = ((colred[0][tid] + colred[1][tid]) + colred[2][tid]) + colred[3][tid];
            }
        }
    }
}

// OUT[:, slot] block a = the fixed-order walk of slab column blockIdx.y (one segment: all tile rows), the four phases in order q = 0..3
__global__ __launch_bounds__(1024) void symm_reduce_kernel(const double *__restrict__ slab, int64_t nb, double *__restrict__ out,
                                                           int64_t ldw, const int *__restrict__ nlive, int ch) {
    const int slot = ch * BQ_SYMM_CK + (int)blockIdx.y;
    if (slot >= *nlive) return;
    __shared__ double part[4][ST];
    const int64_t a = blockIdx.x;
    const int r = threadIdx.x & (ST - 1), q = threadIdx.x >> 8;
    part[q][r] = seg_thread_sum<SJG>(slab + ((int64_t)blockIdx.y * nb + a) * nb * ST + r, a, 0, nb, q);
    __syncthreads();
    if (q == 0) out[slot * ldw + a * ST + r] = ((part[0][r] + part[1][r]) + part[2][r]) + part[3][r];
}

int64_t bq_symm_slab_len(int64_t nb) { return (int64_t)BQ_SYMM_CK * nb * nb * ST; }

int bq_launch_symm(bq_problem *p, bool add_one, const double *W, int64_t ldw, int slots, double *slab, double *out,
                   const int *nlive) {
    BQ_ARG(p->symmetric && !p->streamed && p->ctx->world == 1, "the multi-column product needs a resident packed panel on one rank");
    BQ_ARG(ldw >= p->nb * ST, "column stride shorter than the panel");
    const int64_t nb = p->nb;
    const dim3 tiles((unsigned)strips_before<SJG>(nb)), red((unsigned)nb, BQ_SYMM_CK);
    hipStream_t st = p->ctx->stream;
    for (int ch = 0; ch * BQ_SYMM_CK < slots; ++ch) {
        bq_panel_dispatch(p, add_one, [&](auto pv, auto one) {
            symm_tiles_kernel<bq_pelem<decltype(pv)>, decltype(one)::value><<<tiles, 256, 0, st>>>(pv, nb, W, ldw, slab, nlive, ch);
        });
        symm_reduce_kernel<<<red, 1024, 0, st>>>(slab, nb, out, ldw, nlive, ch);
        BQ_HIP(hipGetLastError());
    }
    return BQ_OK;
}

int bq_product_once(bq_problem *p, const char *name, int k, int64_t slots, int64_t slab_len, bool zero_out, const double *W,
                    double *out, bq_product_launch launch, void *arg) {
    bq_ctx *c = p->ctx;
    const int64_t ldw = p->ldN;
    bq_scratch mem;   // freed after the closing sync
    double *dW = mem.dev<double>(ldw * slots), *dO = mem.dev<double>(ldw * slots), *slab = mem.dev<double>(slab_len);
    int *nl = mem.dev<int>(1);
    hipError_t e = mem.error();
    if (e == hipSuccess) e = hipMemsetAsync(dW, 0, sizeof(double) * ldw * slots, c->stream);
    if (e == hipSuccess && zero_out) e = hipMemsetAsync(dO, 0, sizeof(double) * ldw * slots, c->stream);
    if (e == hipSuccess) e = hipMemcpy2DAsync(dW, sizeof(double) * ldw, W, sizeof(double) * p->n, sizeof(double) * p->n, k,
                                              hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(nl, &k, sizeof(int), hipMemcpyHostToDevice, c->stream);
    int rc = BQ_OK;
    if (e != hipSuccess) {
        bq_set_error("%s setup failed: %s", name, hipGetErrorString(e));
        rc = e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
    }
    if (rc == BQ_OK) rc = launch(arg, dW, ldw, slab, dO, nl);
    if (rc == BQ_OK) {
        e = hipMemcpy2DAsync(out, sizeof(double) * p->n, dO, sizeof(double) * ldw, sizeof(double) * p->n, k, hipMemcpyDeviceToHost,
                             c->stream);
        if (e != hipSuccess) {
            bq_set_error("%s copy: %s", name, hipGetErrorString(e));
            rc = BQ_ERR_HIP;
        }
    }
    return bq_ctx_sync_after(c, rc);
}

static int gram_matmat(bq_problem *p, int k, const double *W, double *out, bool wide) {
    BQ_ARG(p && W && out, "NULL argument");
    BQ_ARG(k >= 1, "k must be >= 1");
    BQ_ARG(p->kernel >= 0, "not a kernel-structured problem");
    BQ_TRY(bq_need_resident_panel(p, "the multi-column product"));
    BQ_HIP(hipSetDevice(p->ctx->device));
    struct call { bq_problem *p; int k; bool wide; } cl{p, k, wide};
    return bq_product_once(
        p, "gram_matmat", k, bq_round_up(k, wide ? BQ_SYMMW_CK : BQ_SYMM_CK), wide ? bq_symmw_slab_len(p->nb) : bq_symm_slab_len(p->nb),
        false, W, out,
        [](void *arg, const double *dW, int64_t ldw, double *slab, double *dO, const int *nl) {
            const call *c = (const call *)arg;
            return c->wide ? bq_launch_symmw(c->p, false, dW, ldw, c->k, slab, dO, nl)
                           : bq_launch_symm(c->p, false, dW, ldw, c->k, slab, dO, nl);
        },
        &cl);
}

extern "C" int bq_problem_gram_matmat(bq_problem *p, int k, const double *W, double *out) { return gram_matmat(p, k, W, out, false); }

extern "C" int bq_problem_gram_matmat_wide(bq_problem *p, int k, const double *W, double *out) {
    return gram_matmat(p, k, W, out, true);
}
