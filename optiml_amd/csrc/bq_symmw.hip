// Wide multi-column symmetric panel product: OUT[:, s] = P W[:, s] (P = K or K + 1, the packed lower-triangle panel of bq_symv.hip)
// for the slots s < *nlive of W, streaming the panel ONCE per chunk of BQ_SYMMW_CK = 16 columns on the fp64 matrix cores
// (v_mfma_f64_16x16x4_f64, N = 16 = the column chunk).  A cross-validated search puts every (fold, C, class) on one panel
// (svm/model_selection.py), i.e. tens of columns; bq_symm.hip's VALU product takes 4 per stream.
//
// Per stored tile K_IJ (256 x 256) the product needs out_I += K_IJ W_J (row part) and, off the diagonal, out_J += K_IJ' W_I (column
// part).  The MFMA's A operand of lane l is [row l&15][k l>>4], so the two products want the tile fragment in transposed lane layouts:
// the row part takes it as loaded, the column part reads it back transposed from LDS.  Every panel byte is loaded from HBM once.
//
// Blocking: a workgroup (4 waves) streams a STRIP of WJG = 4 consecutive tiles of one tile row; wave w owns tile rows [64w, 64w+64).
// A STEP is one 16 x 64 sub-block of a wave: rows 64w + 16st + (l&15), columns 64cq + f(t, l>>4) of tile column quarter cq; lane l
// loads 16 elements of its row (f64: 8 x 16 B, f32: 4 x 16 B, non-temporal; every instruction reads 64 contiguous bytes of 16 rows).
//   row part     acc1[st] += sum_t mfma(K[..][f(t)], W_J[f(t)][s]), t = 0..15   (W_J staged in LDS per tile; acc1 spans the strip)
//   column part  the sub-block goes to the wave's own LDS image; acc2[jc] += sum_u mfma(K[4u + (l>>4)][16jc + (l&15)], W_I[..][s]),
//                u, jc = 0..3 (W_I in registers for the whole strip); after the 4 steps of a quarter the 4 waves' partials are added
//                in the fixed order w = 0..3 through LDS and written to the slab.
// The f64 MFMA's C/D map is col = lane&15 (= the slot s), row = (lane>>4) + 4 reg.  The next step's loads are issued before the
// current step's MFMAs.
// Slab (bq_symm.hip's layout, 16 columns): a column part per off-diagonal tile and a row part per strip, 2 KiB x 16 each, i.e.
// 1/16 + 1/(16 WJG) of the tile's fp64 bytes each way per chunk.
//
// Determinism and batch invariance: an MFMA output element D[i][s] depends on column s of B only, and every column's chain (the
// t / u / step / tile order, the fixed four-wave sum, seg_thread_sum's walk) is the same for every slot and every chunk; no atomics.
// So column s's bits are a function of W[:, s] alone — alone, at any position, in any batch.  They are not the bits of bq_symm.hip
// or bq_symv.hip (another association); they agree to rounding.
#include "bq_common.h"
#include "bq_symv_tile.h"
#include "bq_symmw_step.h"
using namespace bq_mfma;

// WJG = 4 tiles per strip, CK, and the LDS pitches TP / RP / WP: bq_symmw_step.h (bq_symmp.hip uses the same blocking)
template <typename T, bool ADD_ONE>
__global__ __launch_bounds__(256, 2) void symmw_tiles_kernel(bq_pptr<T> panel, int64_t nb, const double *__restrict__ W,
                                                          int64_t ldw, double *__restrict__ slab, const int *__restrict__ nlive, int ch) {
    const int live = *nlive - ch * CK;   // live slots of this chunk
    if (live <= 0) return;
    __shared__ double tb[4][16 * TP];
    __shared__ double wj[ST * WP];
    const int64_t sidx = (int64_t)blockIdx.x;
    int64_t I = (int64_t)sqrt(2.0 * (double)WJG * (double)sidx);
    if (I >= nb) I = nb - 1;
    while (I > 0 && strips_before<WJG>(I) > sidx) --I;
    while (strips_before<WJG>(I + 1) <= sidx) ++I;
    const int64_t J0 = (sidx - strips_before<WJG>(I)) * WJG;
    const int nj = (int)((J0 + WJG <= I + 1) ? WJG : (I + 1 - J0));

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 4, s = lane & 15;
    // packed layout (bq_sym_addr): WJG tiles from a multiple of WJG lie inside ONE strip of the layout, whose pitch their rows have
    static_assert(BQ_SYM_STRIP % WJG == 0, "a strip of this kernel lies inside one strip of the layout");
    const int64_t gl = J0 / BQ_SYM_STRIP, pitch = bq_sym_strip_w(I, gl);
    const double *Wc = W + (int64_t)ch * CK * ldw;
    const int64_t cs = nb * nb * ST;   // slab stride of one column
    // this wave's row r of tile (I, J0 + j), quarter cq, step st: lane row = 64 wv + 16 st + (lane & 15)
    const auto base = panel + bq_sym_strip_off(I, gl) + (int64_t)(wv * 64 + s) * pitch + (J0 - gl * BQ_SYM_STRIP) * ST;
    auto rowp = [&](int j, int cq, int st) { return base + (int64_t)(16 * st) * pitch + j * ST + 64 * cq; };

    double wi[4][4];   // W_I[64 wv + 16 st + 4 u + h][s]
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
        for (int u = 0; u < 4; ++u) wi[st][u] = Wc[s * ldw + I * ST + wv * 64 + 16 * st + 4 * u + h];
    d4_t acc1[4];
#pragma unroll
    for (int st = 0; st < 4; ++st) acc1[st] = (d4_t){0.0, 0.0, 0.0, 0.0};
    double *img = tb[wv];

    typename step_ld<T>::raw cur, nxt;
    step_ld<T>::load(rowp(0, 0, 0), h, cur);
    const int nquart = nj * 4;
#pragma unroll 1
    for (int qk = 0; qk < nquart; ++qk) {   // quarter cq of tile J0 + j
        const int j = qk >> 2, cq = qk & 3;
        const bool diag = J0 + j == I;   // uniform across the workgroup
        if (cq == 0) {   // stage W_J of the new tile: wj[r][slot]
            __syncthreads();
            const double *wJ = Wc + (J0 + j) * ST + tid;
#pragma unroll
            for (int c = 0; c < CK; ++c) wj[tid * WP + c] = wJ[c * ldw];
            __syncthreads();
        }
        d4_t acc2[4];
#pragma unroll
        for (int jc = 0; jc < 4; ++jc) acc2[jc] = (d4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            if (st < 3) step_ld<T>::load(rowp(j, cq, st + 1), h, nxt);
            else if (qk + 1 < nquart) step_ld<T>::load(rowp((qk + 1) >> 2, (qk + 1) & 3, 0), h, nxt);
            double a[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                a[t] = step_ld<T>::get(cur, t);
                if (ADD_ONE) a[t] += 1.0;
            }
            // row part: A = K[16 rows][f(t, h)], B = W_J[64 cq + f(t, h)][s]
#pragma unroll
            for (int t = 0; t < 16; ++t) acc1[st] = mfma64(a[t], wj[(64 * cq + step_ld<T>::f(t, h)) * WP + s], acc1[st]);
            if (!diag) {
                // column part: the sub-block to this wave's image [row][col], read back as A = K'[16 cols][4 rows]
#pragma unroll
                for (int t = 0; t < 16; t += 2)
                    *reinterpret_cast<d2_t *>(img + s * TP + step_ld<T>::f(t, h)) = (d2_t){a[t], a[t + 1]};
                wave_sync();
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int jc = 0; jc < 4; ++jc) acc2[jc] = mfma64(img[(4 * u + h) * TP + 16 * jc + s], wi[st][u], acc2[jc]);
                wave_sync();
            }
            cur = nxt;
        }
        if (!diag) {   // the quarter's column part: waves' partials -> LDS -> fixed-order sum -> slab
#pragma unroll
            for (int jc = 0; jc < 4; ++jc)
#pragma unroll
                for (int r = 0; r < 4; ++r) img[s * RP + 16 * jc + h + 4 * r] = acc2[jc][r];
            __syncthreads();
            const int c = tid & 63, sg = tid >> 6;
            double *dst = slab + ((J0 + j) * nb + I) * ST + 64 * cq + c;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int sl = 4 * sg + e;
                if (sl < live) dst[sl * cs] = ((tb[0][sl * RP + c] + tb[1][sl * RP + c]) + tb[2][sl * RP + c]) + tb[3][sl * RP + c];
            }
            __syncthreads();
        }
    }
    // row parts of the strip: D[row h + 4 r][slot s] of step st = tile row 64 wv + 16 st + h + 4 r
    if (s < live) {
        double *dst = slab + s * cs + (I * nb + J0) * ST + wv * 64;
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[16 * st + h + 4 * r] = acc1[st][r];
    }
}

// OUT[:, slot] block a = the fixed-order walk of slab column blockIdx.y (one segment: all tile rows), the four phases in order q = 0..3
__global__ __launch_bounds__(1024) void symmw_reduce_kernel(const double *__restrict__ slab, int64_t nb, double *__restrict__ out,
                                                            int64_t ldw, const int *__restrict__ nlive, int ch) {
    const int slot = ch * CK + (int)blockIdx.y;
    if (slot >= *nlive) return;
    __shared__ double part[4][ST];
    const int64_t a = blockIdx.x;
    const int r = threadIdx.x & (ST - 1), q = threadIdx.x >> 8;
    part[q][r] = seg_thread_sum<WJG>(slab + ((int64_t)blockIdx.y * nb + a) * nb * ST + r, a, 0, nb, q);
    __syncthreads();
    if (q == 0) out[slot * ldw + a * ST + r] = ((part[0][r] + part[1][r]) + part[2][r]) + part[3][r];
}

int64_t bq_symmw_slab_len(int64_t nb) { return (int64_t)CK * nb * nb * ST; }

int bq_launch_symmw(bq_problem *p, bool add_one, const double *W, int64_t ldw, int slots, double *slab, double *out,
                    const int *nlive) {
    BQ_ARG(p->symmetric && !p->streamed && p->ctx->world == 1, "the multi-column product needs a resident packed panel on one rank");
    BQ_ARG(ldw >= p->nb * ST, "column stride shorter than the panel");
    const int64_t nb = p->nb;
    const dim3 tiles((unsigned)strips_before<WJG>(nb)), red((unsigned)nb, CK);
    hipStream_t st = p->ctx->stream;
    for (int ch = 0; ch * CK < slots; ++ch) {
        bq_panel_dispatch(p, add_one, [&](auto pv, auto one) {
            symmw_tiles_kernel<bq_pelem<decltype(pv)>, decltype(one)::value><<<tiles, 256, 0, st>>>(pv, nb, W, ldw, slab, nlive, ch);
        });
        symmw_reduce_kernel<<<red, 1024, 0, st>>>(slab, nb, out, ldw, nlive, ch);
        BQ_HIP(hipGetLastError());
    }
    return BQ_OK;
}

extern "C" int64_t bq_problem_wide_slab_bytes(const bq_problem *p) {
    return p == nullptr ? 0 : (int64_t)sizeof(double) * bq_symmw_slab_len(p->nb);
}
