// Symmetric panel product: out = K w reading only the tiles on or below the diagonal — half the HBM bytes of the
// row-block product for the (symmetric) Gram panels of the SVM dual.
//
// The panel is cut into 256 x 256 tiles (I, J), J <= I, and stored PACKED: tile row I keeps only its (I+1)*256 leading
// columns, so the lower triangle costs half the HBM of the square panel.  A work item is a STRIP: up to JG consecutive tiles of one
// tile row, i.e. 256 rows x (JG * 2 KiB) contiguous bytes per row — and the layout stores a strip as ONE row-major block
// (bq_sym_layout.h), so the workgroup reads one contiguous run of up to 4 MiB.  The workgroup streams the strip once (16-byte
// non-temporal loads, lanes along the columns) and produces BOTH contributions the strip is responsible for:
//   row part   S[I][J0][r]  = sum over the strip's columns of elem(K[I*T+r][c]) * w[c]        (to output block I)
//   col parts  S[J][I][c]   = sum_r elem(K[I*T+r][J*T+c]) * w[I*T+r],  each J != I of the strip  (to output block J)
// into a slab S[nb][nb][T]; a second kernel sums the slab entries of each output block in a fixed order ->
// deterministic, no atomics.  Column sums are lane-local (a lane owns 4 columns of every tile); the row partials of a
// step are accumulated over the whole strip and then reduced across the 64 lanes with a halving butterfly
// (4 row sums in 7 shuffle-adds).  Slab traffic is about n^2*8/T*(1/2 + 1/(2 JG)) bytes each way (~1 % of the tile bytes).
//
// Multi-GPU: the tile rows are cut into S canonical SEGMENTS with equal shares of the triangle's tiles (bq_common.h); a rank
// owns a contiguous run of segments and produces, per segment, a partial vector for every output block.  One in-place
// all-gather per product hands every rank all S segment vectors, which are then added in segment order — the same
// association for any rank count, so 1/2/4/8-GPU iterates are bit-identical.  (BQ_SYM_EXCHANGE=allreduce: each rank adds
// its own segments and the rank partials meet in one ncclAllReduce — the sum's association then depends on the ring.)
//
// Shared with the other product files: the storage dispatch of the launchers (bq_panel_dispatch, bq_c7.h; launch_tiles hands it the
// timed launch, and the compact layout at 8 rows per step, which is not built, is an error there) and the fixed-order walk of a slab
// column (slab_walk under seg_thread_sum, bq_symv_tile.h).  The strip body of symv_tiles_kernel is its own: bq_symmp.hip's single
// kernel repeats it, because as one inlined function template this kernel compiled to other code than it has alone.
#include <algorithm>
#include <cstdlib>

#include <hip/hip_ext.h>

#include "bq_common.h"
#include "bq_epilogue.h"
#include "bq_symv_tile.h"

constexpr int JG_DEFAULT = 8;   // tiles per strip (8 x 2 KiB contiguous per row; best of the measured variants)

// One workgroup of four waves streams all 256 rows of a strip: wave `wv` owns rows [64 wv, 64 wv + 64).
// (Round 4 also carried a row-cut variant — two 128-thread workgroups per strip with a three-entry column slab — for short grids: built,
// bit-identical, measured no faster (1/8 shares 0.796 - 0.885 ms cut against 0.801 - 0.832 ms uncut, profiles/r04/symv_row_cut_strips.txt)
// and removed in round 5 together with the <4,4> <4,8> <2,8> <2,4> tuning variants: HISTORY.md.)
template <typename T, bool ADD_ONE, int JG, int SR>
__global__ __launch_bounds__(256, 2) void symv_tiles_kernel(bq_pptr<T> panel, int64_t I0, int64_t nb,
                                                          const double *__restrict__ w, double *__restrict__ slab,
                                                          const int *__restrict__ done, int *__restrict__ skip, int skip_seq) {
    if (done != nullptr && *done) {
        if (skip != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *skip = skip_seq;   // bq_prof_skip_arg: "this launch was no product"
        return;
    }
    __shared__ double colred[4][ST];
    // decode (I, g) from the linear strip index
    const int64_t t = (int64_t)blockIdx.x + strips_before<JG>(I0);
    int64_t I = (int64_t)sqrt(2.0 * (double)JG * (double)t);
    if (I >= nb) I = nb - 1;
    while (I > 0 && strips_before<JG>(I) > t) --I;
    while (strips_before<JG>(I + 1) <= t) ++I;
    const int64_t g = t - strips_before<JG>(I);
    const int64_t J0 = g * JG;
    const int nj = (int)((J0 + JG <= I + 1) ? JG : (I + 1 - J0));  // tiles in this strip (J <= I)

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // packed symmetric layout (bq_sym_addr): the strip is one contiguous row-major 256 x (nj * 256) block.  The wave's first row is
    // told to the compiler as the wave-uniform value it is: the strip base and every row offset then stay in scalar registers (with
    // the wave index in a vector register the 8-row and the compact instantiations spilled: profiles/strip_layout).
    static_assert(JG == BQ_SYM_STRIP, "the strip of the kernel is the strip of the layout");
    const int64_t pitch = bq_sym_strip_w(I, g);
    const auto rows = panel + ((bq_sym_strip_off(I, g) - bq_sym_off(I0)) + (int64_t)(__builtin_amdgcn_readfirstlane(wv) * 64) * pitch);
    const double *wI = w + I * ST + wv * 64;
    const int c0 = tile_ld<T>::c0(lane), c1 = tile_ld<T>::c1(lane);
    d2_t wj0[JG], wj1[JG];
    double ca[JG][4];
#pragma unroll
    for (int j = 0; j < JG; ++j) {
        const double *wJ = w + (J0 + (j < nj ? j : 0)) * ST;
        wj0[j] = *reinterpret_cast<const d2_t *>(wJ + c0);
        wj1[j] = *reinterpret_cast<const d2_t *>(wJ + c1);
        ca[j][0] = ca[j][1] = ca[j][2] = ca[j][3] = 0.0;
    }
    double *rowout = slab + (I * nb + J0) * ST + wv * 64;
    const bool b5 = lane & 32, b4 = lane & 16;

#pragma unroll 1
    for (int step = 0; step < 64 / SR; ++step) {
        double rp[SR];
        double wi[SR];
#pragma unroll
        for (int k = 0; k < SR; ++k) {
            rp[k] = 0.0;
            wi[k] = wI[step * SR + k];
        }
#pragma unroll
        for (int j = 0; j < JG; ++j) {
            if (j < nj) {
                d2_t a[SR], b[SR];
#pragma unroll
                for (int k = 0; k < SR; ++k) {
                    const auto row = rows + (int64_t)(step * SR + k) * pitch + j * ST;
                    tile_ld<T>::get(row, lane, a[k], b[k]);
                }
                tile_post<T>::issued();
#pragma unroll
                for (int k = 0; k < SR; ++k) {
                    tile_post<T>::decode(a[k], b[k]);
                    if (ADD_ONE) {
                        a[k].x += 1.0;
                        a[k].y += 1.0;
                        b[k].x += 1.0;
                        b[k].y += 1.0;
                    }
                    rp[k] = fma(b[k].y, wj1[j].y, fma(b[k].x, wj1[j].x, fma(a[k].y, wj0[j].y, fma(a[k].x, wj0[j].x, rp[k]))));
                    ca[j][0] = fma(a[k].x, wi[k], ca[j][0]);
                    ca[j][1] = fma(a[k].y, wi[k], ca[j][1]);
                    ca[j][2] = fma(b[k].x, wi[k], ca[j][2]);
                    ca[j][3] = fma(b[k].y, wi[k], ca[j][3]);
                }
            }
        }
        // halving butterfly: SR row partials x 64 lanes -> one full row sum per (64 / SR)-lane group
        double s1;
        int rho;
        if constexpr (SR == 8) {
            const bool b3 = lane & 8;
            double u[4], t2[2];
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
            rho = (b5 ? 4 : 0) + (b4 ? 2 : 0) + (b3 ? 1 : 0);
        } else {
            static_assert(SR == 4 || SR == 8, "SR");
            double u[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const double send = b5 ? rp[i] : rp[i + 2];
                const double keep = b5 ? rp[i + 2] : rp[i];
                u[i] = keep + __shfl_xor(send, 32, 64);
            }
            {
                const double send = b4 ? u[0] : u[1];
                const double keep = b4 ? u[1] : u[0];
                s1 = keep + __shfl_xor(send, 16, 64);
            }
            s1 += __shfl_xor(s1, 8, 64);
            rho = (b5 ? 2 : 0) + (b4 ? 1 : 0);
        }
        s1 += __shfl_xor(s1, 4, 64);
        s1 += __shfl_xor(s1, 2, 64);
        s1 += __shfl_xor(s1, 1, 64);
        if ((lane & (64 / SR - 1)) == 0) rowout[step * SR + rho] = s1;
    }
    // column parts of every off-diagonal tile of the strip
#pragma unroll
    for (int j = 0; j < JG; ++j) {
        if (j < nj && J0 + j != I) {   // uniform across the workgroup
            __syncthreads();
            colred[wv][c0] = ca[j][0];
            colred[wv][c0 + 1] = ca[j][1];
            colred[wv][c1] = ca[j][2];
            colred[wv][c1 + 1] = ca[j][3];
            __syncthreads();
            const int64_t entry = (J0 + j) * nb + I;
            slab[entry * ST + tid] = ((colred[0][tid] + colred[1][tid]) + colred[2][tid]) + colred[3][tid];
        }
    }
}

// the four phases of a segment's sum combined in the fixed order q = 0..3; every thread returns the combined value
template <int JG>
__device__ __forceinline__ double seg_partial(const double *__restrict__ p, int64_t a, int64_t c0, int64_t c1, int q, int r,
                                              double (*part)[ST]) {
    part[q][r] = seg_thread_sum<JG>(p, a, c0, c1, q);
    __syncthreads();
    const double v = ((part[0][r] + part[1][r]) + part[2][r]) + part[3][r];
    __syncthreads();
    return v;
}

// out[a*T + r] = sum over the segments [tab.lo, tab.hi) of their partial sums, in segment order — the canonical order of
// the product: the same association whether the segments were summed here (one rank) or gathered from their owners
// EPI: the PG / FW epilogue of bq_epilogue.h goes on from the summed product (out is still written: other consumers read p->s)
template <int JG, int EPI>
__global__ __launch_bounds__(1024) void symv_reduce_kernel(const double *__restrict__ slab, int64_t nb, bq_seg_table tab,
                                                           double *__restrict__ out, const int *__restrict__ done, bq_epilogue epi) {
    if (done != nullptr && *done) return;
    // the phase sums of up to eight segments (all of them on one rank) meet in LDS in ONE round of barriers — one round per segment
    // made sixteen barriers of 1 024 threads, a third of this kernel's length; the association per segment and the segment order
    // of the final sum are what they were
    __shared__ double part[BQ_SYM_SEG][4][ST];
    const int64_t a = blockIdx.x;
    const int r = threadIdx.x & (ST - 1), q = threadIdx.x >> 8;
    const double *p = slab + a * nb * ST + r;
    bq_epi_pre pre;
    bq_al_pre apre;
    if constexpr (EPI == BQ_EPI_PGFW) pre = bq_epi_preload(epi, a * ST + r, q == 0);   // in flight while the slab is walked
    if constexpr (EPI == BQ_EPI_AL) apre = bq_al_epi_preload(epi, a * ST + r, q == 0, true);
    double acc = 0.0;
    for (int s0 = tab.lo; s0 < tab.hi; s0 += BQ_SYM_SEG) {
        const int ns = tab.hi - s0 < BQ_SYM_SEG ? tab.hi - s0 : BQ_SYM_SEG;
        for (int k = 0; k < ns; ++k) part[k][q][r] = seg_thread_sum<JG>(p, a, tab.cut[s0 + k], tab.cut[s0 + k + 1], q);
        __syncthreads();
        if (q == 0)
            for (int k = 0; k < ns; ++k) acc += ((part[k][0][r] + part[k][1][r]) + part[k][2][r]) + part[k][3][r];
        __syncthreads();
    }
    if (q == 0) out[a * ST + r] = acc;
    if constexpr (EPI == BQ_EPI_PGFW) bq_epi_finish(epi, a, nb, bq_epi_element(epi, pre, a * ST + r, acc), gridDim.x);
    if constexpr (EPI == BQ_EPI_AL) bq_al_epi_finish<true>(epi, a, nb, bq_al_epi_element(epi, apre, a * ST + r, acc, true), gridDim.x);
}

// the per-segment partial vectors of this rank's segments, each to its slot of the gathered buffer
template <int JG>
__global__ __launch_bounds__(1024) void symv_reduce_seg_kernel(const double *__restrict__ slab, int64_t nb, bq_seg_table tab,
                                                               double *__restrict__ gath, const int *__restrict__ done) {
    if (done != nullptr && *done) return;
    __shared__ double part[4][ST];
    const int64_t a = blockIdx.x;
    const int s = tab.lo + (int)blockIdx.y;
    const int r = threadIdx.x & (ST - 1), q = threadIdx.x >> 8;
    const double v = seg_partial<JG>(slab + a * nb * ST + r, a, tab.cut[s], tab.cut[s + 1], q, r, part);
    if (q == 0) gath[((int64_t)tab.slot[s] * nb + a) * ST + r] = v;
}

// out = sum of all S gathered segment vectors in segment order (every rank: identical bits); EPI: as symv_reduce_kernel
template <int EPI>
__global__ __launch_bounds__(256) void symv_segsum_kernel(const double *__restrict__ gath, int64_t len, bq_seg_table tab,
                                                          double *__restrict__ out, const int *__restrict__ done, bq_epilogue epi) {
    if (done != nullptr && *done) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // len = nb * 256: always in range
    bq_epi_pre pre;
    bq_al_pre apre;
    if constexpr (EPI == BQ_EPI_PGFW) pre = bq_epi_preload(epi, i, true);
    if constexpr (EPI == BQ_EPI_AL) apre = bq_al_epi_preload(epi, i, true, true);
    double acc = 0.0;
    int s = 0;
    for (; s + 8 <= tab.count; s += 8) {   // the canonical eight segments: eight loads in flight, added in segment order
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = gath[(int64_t)tab.slot[s + u] * len + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; s < tab.count; ++s) acc += gath[(int64_t)tab.slot[s] * len + i];
    out[i] = acc;
    if constexpr (EPI == BQ_EPI_PGFW) bq_epi_finish(epi, blockIdx.x, gridDim.x, bq_epi_element(epi, pre, i, acc), gridDim.x);
    if constexpr (EPI == BQ_EPI_AL) bq_al_epi_finish<true>(epi, blockIdx.x, gridDim.x, bq_al_epi_element(epi, apre, i, acc, true), gridDim.x);
}

// The timed launch: when the context is profiling, the kernel's own dispatch carries the two timestamps (hipExtLaunchKernelGGL with a
// start and a stop event) instead of two events recorded around it on the stream: the duration is the kernel's own, as rocprofv3's
// kernel trace reports it, and the stream carries nothing a solve without profiling would not (measured: 1-2 us per product less than
// the bracketing, profiles/r04/share_gaps_events.txt).
template <typename K, typename... A>
static hipError_t launch_timed(bq_ctx *ctx, bool ext, hipEvent_t e0, hipEvent_t e1, K kernel, dim3 grid, dim3 block, A... args) {
    if (ext)
        hipExtLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, e0, e1, 0, args...);
    else
        kernel<<<grid, block, 0, ctx->stream>>>(args...);
    return hipGetLastError();
}

template <int JG, int SR>
static int launch_tiles(bq_ctx *ctx, const bq_panel_ref &panel, bool add_one, int64_t I0, int64_t I1, int64_t nb,
                        const double *w, double *slab, const int *done) {
    constexpr bool bracket = false;   // (round 4's BQ_PROF_BRACKET=1 — events recorded around the launch — cost 1-2 us per product: removed)
    const int64_t nstrips = strips_before<JG>(I1) - strips_before<JG>(I0);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    BQ_TRY(bq_prof_begin(ctx, BQ_PROF_MATVEC, &e0, &e1, bracket));
    if (nstrips <= 0) {
        if (!bracket) {
            bq_prof_drop(ctx, e0, e1);
            return BQ_OK;
        }
        return bq_prof_end(ctx, BQ_PROF_MATVEC, e0, e1);
    }
    int *skip = nullptr, skip_seq = 0;
    if (done != nullptr) bq_prof_skip_arg(ctx, e0, &skip, &skip_seq);
    const bool ext = !bracket && e0 != nullptr;
    const dim3 grid((unsigned)nstrips), block(256);
    hipError_t err = hipSuccess;
    if (panel.storage == BQ_F64H) {   // the Hessian image (bq_h52.h): its elements are fl(K + 1) already; 4 rows per step as for the compact panel
        if constexpr (SR == 4)
            err = add_one ? hipErrorInvalidValue
                          : launch_timed(ctx, ext, e0, e1, symv_tiles_kernel<bq_h52, false, JG, 4>, grid, block,
                                         bq_h52_view(panel.base, panel.elems), I0, nb, w, slab, done, skip, skip_seq);
        else
            err = hipErrorInvalidValue;
    } else bq_panel_dispatch(panel, add_one, [&](auto pv, auto one) {
        using T = bq_pelem<decltype(pv)>;
        if constexpr (std::is_same<T, bq_c7>::value && SR != 4)
            err = hipErrorInvalidValue;   // not built: launch_any keeps the compact layout at 4 rows per step
        else
            err = launch_timed(ctx, ext, e0, e1, symv_tiles_kernel<T, decltype(one)::value, JG, SR>, grid, block, pv, I0, nb, w, slab,
                               done, skip, skip_seq);
    });
    if (err != hipSuccess) {
        bq_prof_drop(ctx, e0, e1);
        bq_set_error("symv_tiles launch: %s", hipGetErrorString(err));
        return BQ_ERR_HIP;
    }
    return bq_prof_end(ctx, BQ_PROF_MATVEC, e0, e1, ext);
}

// mode 0: tiles + the sum over this launch's segments -> out (nb*256);  mode 1: tiles + one vector per segment -> gath slots
template <int SR>
static int launch_variant(bq_ctx *ctx, const bq_panel_ref &panel, bool add_one, int64_t nb, const bq_seg_table &tab,
                          const double *w, double *slab, double *out, int mode, const int *done, const bq_epilogue *epi) {
    constexpr int JG = JG_DEFAULT;
    BQ_TRY((launch_tiles<JG, SR>(ctx, panel, add_one, tab.cut[tab.lo], tab.cut[tab.hi], nb, w, slab, done)));
    if (mode == 0 && bq_epi_mode(epi) == BQ_EPI_PGFW)
        symv_reduce_kernel<JG, BQ_EPI_PGFW><<<(unsigned)nb, 1024, 0, ctx->stream>>>(slab, nb, tab, out, done, *epi);
    else if (mode == 0 && bq_epi_mode(epi) == BQ_EPI_AL)
        symv_reduce_kernel<JG, BQ_EPI_AL><<<(unsigned)nb, 1024, 0, ctx->stream>>>(slab, nb, tab, out, done, *epi);
    else if (mode == 0)
        symv_reduce_kernel<JG, BQ_EPI_NONE><<<(unsigned)nb, 1024, 0, ctx->stream>>>(slab, nb, tab, out, done, bq_epilogue{});
    else if (tab.hi > tab.lo)
        symv_reduce_seg_kernel<JG><<<dim3((unsigned)nb, (unsigned)(tab.hi - tab.lo)), 1024, 0, ctx->stream>>>(slab, nb, tab, out, done);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

static int launch_any(bq_ctx *ctx, const bq_panel_ref &panel, bool add_one, int64_t nb, const bq_seg_table &tab,
                      const double *w, double *slab, double *out, int mode, const int *done, const bq_epilogue *epi = nullptr) {
    // Rows per step (loads in flight per wave).  fp32 tiles are half as wide in bytes: 8 rows per step keep the same bytes in
    // flight per lane.  fp64: 4 rows per step, except on short grids whose LAST round of workgroups is sparsely filled (two
    // workgroups per CU = 512 slots on this chip; a 1/8 share of n = 100 000 is ~1 200 strips = 2.3 rounds): there 8 rows per
    // step keep HBM busy while that round drains.  Measured (profiles/r03/symv_rows_per_step.txt): 1 200 strips 0.85 -> 0.81 ms,
    // 1 650 strips (n = 40 000) 1.07 -> 1.02 ms; grids whose last round is well filled are 2-6 % faster with 4, long grids do not
    // care.  The rows of a step are independent sums and the lane butterfly pairs the same lanes in the same order: the bits do
    // not depend on the choice (tests/test_distributed.py::test_rows_per_step_variants_are_bit_identical).
    const int force = (int)bq_hook_value("rows_per_step", 0.0);   // 4 or 8: no heuristic (the bit-identity test switches it)
    const int64_t strips = strips_before<JG_DEFAULT>(tab.cut[tab.hi]) - strips_before<JG_DEFAULT>(tab.cut[tab.lo]);
    const int64_t slots = 2 * (int64_t)(ctx->num_cu > 0 ? ctx->num_cu : 256);
    const bool sparse_tail = strips >= slots && strips < 8 * slots && 2 * (strips % slots) < slots;
    // The compact layout (bq_c7.h) always takes 4: its decode makes the 8-row step spill (12 bytes per lane of scratch).
    const bool eight = panel.storage != BQ_F64C && panel.storage != BQ_F64H && (force == 8 || (force != 4 && (panel.storage == BQ_F32 || sparse_tail)));
    if (eight) return launch_variant<8>(ctx, panel, add_one, nb, tab, w, slab, out, mode, done, epi);
    return launch_variant<4>(ctx, panel, add_one, nb, tab, w, slab, out, mode, done, epi);
}

// The writer of the Hessian image (bq_h52.h).  Every aligned run of 256 packed indices is one row of one tile (bq_sym_layout.h), so the
// conversion needs no tile geometry: a wave takes one run, lane l reads the column pairs {2l, 2l + 1} and {128 + 2l, 129 + 2l} through
// the decode the product uses (bq_c7p::pair), adds 1.0 in fp64 — the operand the product's first FMA sees today — and writes the four
// codes to positions 4l .. 4l + 3: one 16-byte, one 8-byte and one 2-byte store.
__global__ __launch_bounds__(256) void h52_convert_kernel(bq_c7p panel, int64_t runs, uint32_t *__restrict__ lo, uint16_t *__restrict__ mid,
                                                          uint8_t *__restrict__ nib, int *__restrict__ bad, int force_bad) {
    typedef unsigned int u4_t __attribute__((ext_vector_type(4)));
    typedef unsigned int u2_t __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    bool any_bad = force_bad != 0 && blockIdx.x == 0 && threadIdx.x == 0;
    for (int64_t run = wave; run < runs; run += nwaves) {
        const int64_t base = run * BQ_H52_ROW;
        const d2_t a = panel.pair(base + 2 * lane), b = panel.pair(base + 128 + 2 * lane);
        const double h[4] = {a.x + 1.0, a.y + 1.0, b.x + 1.0, b.y + 1.0};
        uint64_t c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] = bq_h52_encode((uint64_t)__double_as_longlong(h[q]), &any_bad);
        const u4_t l = {(uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2], (uint32_t)c[3]};
        const u2_t m = {((uint32_t)(c[0] >> 32) & 0xFFFFu) | ((uint32_t)(c[1] >> 32) << 16),
                        ((uint32_t)(c[2] >> 32) & 0xFFFFu) | ((uint32_t)(c[3] >> 32) << 16)};
        const uint32_t t = (uint32_t)(c[0] >> 48) | ((uint32_t)(c[1] >> 48) << 4) | ((uint32_t)(c[2] >> 48) << 8) | ((uint32_t)(c[3] >> 48) << 12);
        *reinterpret_cast<u4_t *>(lo + base + 4 * lane) = l;
        *reinterpret_cast<u2_t *>(mid + base + 4 * lane) = m;
        *reinterpret_cast<uint16_t *>(nib + (base >> 1) + 2 * lane) = (uint16_t)t;
    }
    if (any_bad) *bad = 1;
}

int bq_launch_h52_convert(bq_ctx *ctx, const bq_problem *p, void *image, int *bad, bool force_bad) {
    if (!p->compact || p->panel == nullptr || p->panel_elems <= 0 || p->panel_elems % BQ_H52_ROW != 0) {
        bq_set_error("the Hessian image is built from a resident compact panel");
        return BQ_ERR_BADARG;
    }
    BQ_HIP(hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
    const int64_t runs = p->panel_elems / BQ_H52_ROW;
    unsigned char *b = (unsigned char *)image;
    const int64_t blocks = std::min<int64_t>((runs + 3) / 4, 8 * (int64_t)(ctx->num_cu > 0 ? ctx->num_cu : 256));
    h52_convert_kernel<<<(unsigned)blocks, 256, 0, ctx->stream>>>(bq_c7_view(p->panel, p->panel_elems), runs, (uint32_t *)b,
                                                                  (uint16_t *)(b + 4 * p->panel_elems), b + 6 * p->panel_elems, bad,
                                                                  force_bad ? 1 : 0);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

int bq_launch_symv(bq_ctx *ctx, const bq_panel_ref &panel, bool add_one, int64_t nb, const bq_seg_table &tab,
                   const double *w, double *slab, double *out, const int *done, const bq_epilogue *epi) {
    return launch_any(ctx, panel, add_one, nb, tab, w, slab, out, 0, done, epi);
}

int bq_launch_symv_segments(bq_ctx *ctx, const bq_panel_ref &panel, bool add_one, int64_t nb, const bq_seg_table &tab,
                            const double *w, double *slab, double *gath, const int *done) {
    return launch_any(ctx, panel, add_one, nb, tab, w, slab, gath, 1, done);
}

int bq_launch_symv_segsum(bq_ctx *ctx, int64_t nb, const bq_seg_table &tab, const double *gath, double *out, const int *done,
                          const bq_epilogue *epi) {
    const int64_t len = nb * ST;
    if (bq_epi_mode(epi) == BQ_EPI_PGFW)
        symv_segsum_kernel<BQ_EPI_PGFW><<<(unsigned)nb, 256, 0, ctx->stream>>>(gath, len, tab, out, done, *epi);
    else if (bq_epi_mode(epi) == BQ_EPI_AL)
        symv_segsum_kernel<BQ_EPI_AL><<<(unsigned)nb, 256, 0, ctx->stream>>>(gath, len, tab, out, done, *epi);
    else
        symv_segsum_kernel<BQ_EPI_NONE><<<(unsigned)nb, 256, 0, ctx->stream>>>(gath, len, tab, out, done, bq_epilogue{});
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}
