// Pair-routed symmetric panel product for one-vs-one multi-class SVC: OUT[:, p] = P W[:, p] on the rows of classes a and b of
// pair p = (a, b), a < b, and exact 0.0 on every other row, for every live pair at once, streaming the panel ONCE.
//
// The panel's rows are sorted by class and every class owns whole 256-row tile rows: class c is tile rows [ct[c], ct[c + 1]).
// Every stored tile (I, J), J <= I, is then one of two kinds:
//   off-diagonal class block  I of class b, J of class a < b: only pair (a, b) reads it — a one-column tile walk (bq_symv.hip's VALU
//                             scheme: row part to the rows of b with W_a, column part to the rows of a with W_b);
//   diagonal class block      I, J of class c: every live pair containing c reads it — bq_symmw.hip's v_mfma_f64_16x16x4_f64 scheme
//                             over the class's sub-triangle, with the live pairs of c gathered into slots, 16 per chunk.
// The work list (host, built once per plan): per tile row I of class b, one single-column SEGMENT per pair (a, b) over the tiles
// [ct[a], ct[a + 1]) cut into strips of JG tiles, and one diagonal segment over [ct[b], I] cut into strips of WJG tiles.  Liveness is
// read on the device: a strip whose pair, or every slot of whose diagonal chunk, has stopped returns at once (no host sync).  So a
// tile is read from HBM at most once per chunk of 16 columns that use it, and an off-diagonal block of a stopped pair not at all.
//
// Slab: pair p has its own L_p x L_p region of 256-entry vectors, L_p = tiles of a + tiles of b, in pair-local tile numbering (a's
// tiles first).  Entry (A, B): B > A holds the column part of tile (B, A); B <= A holds the row part of the h-th strip of tile row A
// (h = B: row parts are numbered, not placed at their first tile).  The reduce adds row A's row parts in strip order, then its column
// parts in tile order, in four fixed phases (bq_symv_tile.h's slab_walk, as seg_thread_sum) — no atomics.
//
// Determinism and batch invariance: each column's chain (tile walk, MFMA k order, four-wave sum, reduce walk) depends only on its
// pair's class layout and its W column; an MFMA output D[i][s] depends on column s of B only.  So column p's bits are the same
// alone, at any slot, and whatever other pairs are live.  They are not the bits of bq_symmw.hip (another association).
#include <algorithm>
#include <type_traits>
#include <vector>

#include "bq_common.h"
#include "bq_symv_tile.h"
#include "bq_symmw_step.h"
using namespace bq_mfma;

namespace {

constexpr int JG = 8;      // tiles per single-column strip (bq_symv.hip's default); diagonal strips: WJG (bq_symmw_step.h)

struct pitem {
    int I, J0, nj, id;   // tile row, first tile, tiles; single: the pair, diagonal: the class
};
struct pinfo {
    long long base;   // first double of the pair's slab region
    int L, na, ns;    // tiles of the pair, tiles of a, single-column strips per tile row of b
    int a0, b0;       // first tile rows of a and b
};

}  // namespace

struct bq_pairs_plan {
    bq_owner mem;   // the device buffers below
    int ncls = 0, m = 0, kpad = 0, nch = 0, lmax = 0;
    int64_t nb = 0, slab_len = 0, nsingle = 0, ndiag = 0;
    std::vector<int> ct, pairs;
    pitem *single = nullptr, *diag = nullptr;
    pinfo *info = nullptr;
    int *dct = nullptr, *dpairs = nullptr;
    int *plive = nullptr, *ccnt = nullptr, *cslot = nullptr;   // live flag per pair; live pairs per class and their slots
};

static int check_pairs(int64_t nb, int ncls, const int *ct, int m, const int *pairs) {
    BQ_ARG(ct != nullptr && pairs != nullptr, "NULL argument");
    BQ_ARG(ncls >= 2, "ncls must be >= 2");
    BQ_ARG(m >= 1, "m must be >= 1");
    BQ_ARG(ct[0] == 0, "cls_tiles[0] must be 0");
    for (int c = 0; c < ncls; ++c) BQ_ARG(ct[c] < ct[c + 1], "cls_tiles must be strictly increasing");
    BQ_ARG(ct[ncls] == nb, "cls_tiles[ncls] must be the panel's number of tile rows");
    for (int p = 0; p < m; ++p) BQ_ARG(pairs[2 * p] >= 0 && pairs[2 * p] < pairs[2 * p + 1] && pairs[2 * p + 1] < ncls,
                                       "pairs must be (a, b) with 0 <= a < b < ncls");
    return BQ_OK;
}

static void build_lists(int ncls, const int *ct, int m, const int *pairs, std::vector<pitem> &single, std::vector<pitem> &diag,
                        std::vector<int> &cnt) {
    cnt.assign(ncls, 0);
    for (int p = 0; p < m; ++p) {
        cnt[pairs[2 * p]] += 1;
        cnt[pairs[2 * p + 1]] += 1;
    }
    for (int p = 0; p < m; ++p) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        for (int I = ct[b]; I < ct[b + 1]; ++I)
            for (int J0 = ct[a]; J0 < ct[a + 1]; J0 += JG) single.push_back(pitem{I, J0, std::min(JG, ct[a + 1] - J0), p});
    }
    for (int c = 0; c < ncls; ++c) {
        if (cnt[c] == 0) continue;
        for (int I = ct[c]; I < ct[c + 1]; ++I)
            for (int J0 = ct[c]; J0 <= I; J0 += WJG) diag.push_back(pitem{I, J0, std::min(WJG, I + 1 - J0), c});
    }
}

static int64_t slab_len(const int *ct, int m, const int *pairs) {
    int64_t len = 0;
    for (int p = 0; p < m; ++p) {
        const int64_t L = (ct[pairs[2 * p] + 1] - ct[pairs[2 * p]]) + (ct[pairs[2 * p + 1] + 1] - ct[pairs[2 * p + 1]]);
        len += L * L * ST;
    }
    return len;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------------------------

// bq_symv.hip's symv_tiles_kernel on one strip of an off-diagonal class block (every tile off the panel's diagonal), one column.
// The walk is written out here and there: called as one inlined body, symv_tiles_kernel compiles to other code
// (profiles/refactor/isa_diff.txt), and that kernel is the headline product.
template <typename T, bool ADD_ONE, int SR>
__global__ __launch_bounds__(256, 2) void symmp_single_kernel(bq_pptr<T> panel, const pitem *__restrict__ items,
                                                              const pinfo *__restrict__ info, const int *__restrict__ plive,
                                                              const double *__restrict__ W, int64_t ldw, double *__restrict__ slab) {
    const pitem it = items[blockIdx.x];
    if (!plive[it.id]) return;
    __shared__ double colred[4][ST];
    const pinfo pi = info[it.id];
    const int64_t I = it.I, J0 = it.J0;
    const int nj = it.nj;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double *w = W + (int64_t)it.id * ldw;
    const double *wI = w + I * ST + wv * 64;
    const int c0 = tile_ld<T>::c0(lane), c1 = tile_ld<T>::c1(lane);
    d2_t wj0[JG], wj1[JG];
    double ca[JG][4];
    // A class block starts at any tile, so this strip may straddle two strips of the packed layout (bq_sym_addr): tiles j < jsplit lie
    // in layout strip gA, the others in gA + 1, each with its strip's base and row pitch — tile j of this wave's first row is at
    // oA + j * ST or oB + j * ST (all wave-uniform; strip gA + 1 is looked at only when a tile of this strip lies in it)
    static_assert(JG <= BQ_SYM_STRIP, "a strip of this kernel straddles at most two strips of the layout");
    const int64_t gA = J0 / BQ_SYM_STRIP;
    const int jsplit = (int)((gA + 1) * BQ_SYM_STRIP - J0);
    const int64_t pA = bq_sym_strip_w(I, gA), pB = bq_sym_strip_w(I, gA + 1);
    const int64_t wrow = (int64_t)(__builtin_amdgcn_readfirstlane(wv) * 64);
    const int64_t oA = bq_sym_strip_off(I, gA) + wrow * pA + (J0 - gA * BQ_SYM_STRIP) * ST;
    const int64_t oB = bq_sym_strip_off(I, gA + 1) + wrow * pB - jsplit * ST;
#pragma unroll
    for (int j = 0; j < JG; ++j) {
        const int64_t J = J0 + (j < nj ? j : 0);
        const double *wJ = w + J * ST;
        wj0[j] = *reinterpret_cast<const d2_t *>(wJ + c0);
        wj1[j] = *reinterpret_cast<const d2_t *>(wJ + c1);
        ca[j][0] = ca[j][1] = ca[j][2] = ca[j][3] = 0.0;
    }
    const int64_t Il = pi.na + (I - pi.b0), Jl0 = J0 - pi.a0;
    double *ps = slab + pi.base;
    double *rowout = ps + (Il * pi.L + Jl0 / JG) * ST + wv * 64;
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
        int so = step * SR;   // opaque: the row offsets are scalar arithmetic of THIS step (hoisted out of the loop they spill)
        asm volatile("" : "+s"(so));
#pragma unroll
        for (int j = 0; j < JG; ++j) {
            if (j < nj) {
                d2_t a[SR], b[SR];
#pragma unroll
                for (int k = 0; k < SR; ++k) {
                    const int64_t rel = (int64_t)(unsigned)((so + k) * (j < jsplit ? (int)pA : (int)pB) + j * ST);
                    const auto row = panel + ((j < jsplit ? oA : oB) + rel);
                    tile_ld<T>::get(row, lane, a[k], b[k]);
                }
#pragma unroll
                for (int k = 0; k < SR; ++k) {
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
    // column parts: every tile of the strip is off the diagonal
#pragma unroll
    for (int j = 0; j < JG; ++j) {
        if (j < nj) {
            __syncthreads();
            colred[wv][c0] = ca[j][0];
            colred[wv][c0 + 1] = ca[j][1];
            colred[wv][c1] = ca[j][2];
            colred[wv][c1 + 1] = ca[j][3];
            __syncthreads();
            ps[((Jl0 + j) * pi.L + Il) * ST + tid] = ((colred[0][tid] + colred[1][tid]) + colred[2][tid]) + colred[3][tid];
        }
    }
}

// bq_symmw.hip's symmw_tiles_kernel on one strip of class c's diagonal block, the slots being chunk blockIdx.y of c's live pairs.
// Written out in both files: as one inlined body with the slot's column and the slab destinations as callables, the fp32 and fp64
// instantiations took 3 to 8 VGPRs more (of 256 at two waves per SIMD).  The blocking constants are bq_symmw_step.h's.
template <typename T, bool ADD_ONE>
__global__ __launch_bounds__(256, 2) void symmp_diag_kernel(bq_pptr<T> panel, const pitem *__restrict__ items,
                                                            const pinfo *__restrict__ info, const int *__restrict__ pairs,
                                                            const int *__restrict__ ct, const int *__restrict__ ccnt,
                                                            const int *__restrict__ cslot, int kpad, const double *__restrict__ W,
                                                            int64_t ldw, double *__restrict__ slab) {
    const pitem it = items[blockIdx.x];
    const int cls = it.id, ch = blockIdx.y;
    const int live = ccnt[cls] - ch * CK;   // live slots of this chunk
    if (live <= 0) return;
    __shared__ double tb[4][16 * TP];
    __shared__ double wj[ST * WP];
    __shared__ long long sbase[CK];
    __shared__ int sL[CK], soff[CK], shoff[CK], spair[CK];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = lane >> 4, s = lane & 15;
    const int64_t I = it.I, J0 = it.J0, C0 = ct[cls];
    const int nj = it.nj;
    if (tid < CK) {
        int q = -1;
        if (tid < live) {
            q = cslot[cls * kpad + ch * CK + tid];
            const pinfo pi = info[q];
            const bool first = pairs[2 * q] == cls;
            sbase[tid] = pi.base;
            sL[tid] = pi.L;
            soff[tid] = first ? 0 : pi.na;
            shoff[tid] = first ? 0 : pi.ns;
        }
        spair[tid] = q;
    }
    __syncthreads();

    // A class block starts at any tile, so this strip may straddle two strips of the packed layout (bq_sym_addr): the tile of every
    // step is decoded through the address function (uniform), this lane's row within the wave's 64 times the tile's pitch on top
    auto rowp = [&](int j, int cq, int st) {
        const int64_t J = J0 + j, gl = J / BQ_SYM_STRIP, pitch = bq_sym_strip_w(I, gl);
        return panel + (bq_sym_strip_off(I, gl) + (J - gl * BQ_SYM_STRIP) * ST + 64 * cq) + (int64_t)(wv * 64 + 16 * st + s) * pitch;
    };

    const int myq = spair[s];
    double wi[4][4];   // W_I[64 wv + 16 st + 4 u + h][slot s]
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
        for (int u = 0; u < 4; ++u) wi[st][u] = myq >= 0 ? W[(int64_t)myq * ldw + I * ST + wv * 64 + 16 * st + 4 * u + h] : 0.0;
    d4_t acc1[4];
#pragma unroll
    for (int st = 0; st < 4; ++st) acc1[st] = (d4_t){0.0, 0.0, 0.0, 0.0};
    double *img = tb[wv];

    typename step_ld<T>::raw cur, nxt;
    step_ld<T>::load(rowp(0, 0, 0), h, cur);
    const int nquart = nj * 4;
#pragma unroll 1
    for (int qk = 0; qk < nquart; ++qk) {
        const int j = qk >> 2, cq = qk & 3;
        const bool diag = J0 + j == I;
        if (cq == 0) {
            __syncthreads();
            const int64_t r = (J0 + j) * ST + tid;
#pragma unroll
            for (int c = 0; c < CK; ++c) wj[tid * WP + c] = spair[c] >= 0 ? W[(int64_t)spair[c] * ldw + r] : 0.0;
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
#pragma unroll
            for (int t = 0; t < 16; ++t) acc1[st] = mfma64(a[t], wj[(64 * cq + step_ld<T>::f(t, h)) * WP + s], acc1[st]);
            if (!diag) {
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
        if (!diag) {   // column part of tile (I, J0 + j) -> entry (J, I) of every slot's pair
#pragma unroll
            for (int jc = 0; jc < 4; ++jc)
#pragma unroll
                for (int r = 0; r < 4; ++r) img[s * RP + 16 * jc + h + 4 * r] = acc2[jc][r];
            __syncthreads();
            const int c = tid & 63, sg = tid >> 6;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int sl = 4 * sg + e;
                if (sl < live) {
                    const int64_t Jl = soff[sl] + (J0 + j - C0), Il = soff[sl] + (I - C0);
                    slab[sbase[sl] + (Jl * sL[sl] + Il) * ST + 64 * cq + c] =
                        ((tb[0][sl * RP + c] + tb[1][sl * RP + c]) + tb[2][sl * RP + c]) + tb[3][sl * RP + c];
                }
            }
            __syncthreads();
        }
    }
    // row parts of the strip -> entry (I, strip number) of every slot's pair
    if (s < live) {
        const int64_t Il = soff[s] + (I - C0), hh = shoff[s] + (J0 - C0) / WJG;
        double *dst = slab + sbase[s] + (Il * sL[s] + hh) * ST + wv * 64;
#pragma unroll
        for (int st = 0; st < 4; ++st)
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[16 * st + h + 4 * r] = acc1[st][r];
    }
}

// seg_thread_sum's phase rule over the entries [0, nh) then [c0, L) of one slab row (bq_symv_tile.h: slab_walk)
__device__ __forceinline__ double list_sum(const double *__restrict__ p, int64_t nh, int64_t c0, int64_t L, int q) {
    double s0 = 0.0, s1 = 0.0;
    slab_walk(p, q, nh, ST, s0, s1);
    const int64_t shift = (4 - (nh & 3)) & 3;
    slab_walk(p + c0 * ST, (q + shift) & 3, L - c0, ST, s0, s1);
    return s0 + s1;
}

// OUT[:, p] tile A (pair-local) = row A's row parts in strip order, then its column parts in tile order; four phases added q = 0..3
__global__ __launch_bounds__(1024) void symmp_reduce_kernel(const double *__restrict__ slab, const pinfo *__restrict__ info,
                                                            const int *__restrict__ plive, double *__restrict__ out, int64_t ldw) {
    const int p = blockIdx.y;
    if (!plive[p]) return;
    const pinfo pi = info[p];
    const int64_t A = blockIdx.x;
    if (A >= pi.L) return;
    __shared__ double part[4][ST];
    const int r = threadIdx.x & (ST - 1), q = threadIdx.x >> 8;
    const int64_t nh = A < pi.na ? A / WJG + 1 : pi.ns + (A - pi.na) / WJG + 1;
    part[q][r] = list_sum(slab + pi.base + A * pi.L * ST + r, nh, A + 1, pi.L, q);
    __syncthreads();
    const int64_t row = A < pi.na ? pi.a0 + A : pi.b0 + (A - pi.na);
    if (q == 0) out[(int64_t)p * ldw + row * ST + r] = ((part[0][r] + part[1][r]) + part[2][r]) + part[3][r];
}

// the live pairs (not done) and, per class, its live pairs in pair order -> slots; *nlive: their number
__global__ __launch_bounds__(64) void symmp_live_kernel(bq_scal *const *__restrict__ scs, const int *__restrict__ pairs, int m,
                                                       int ncls, int kpad, int *__restrict__ plive, int *__restrict__ ccnt,
                                                       int *__restrict__ cslot, int *__restrict__ nlive) {
    for (int c = threadIdx.x; c < ncls; c += 64) {
        int k = 0;
        for (int p = 0; p < m; ++p)
            if ((pairs[2 * p] == c || pairs[2 * p + 1] == c) && !scs[p]->done) cslot[c * kpad + k++] = p;
        ccnt[c] = k;
    }
    int nl = 0;
    for (int p = 0; p < m; ++p) {
        const int l = !scs[p]->done;
        if (threadIdx.x == 0) plive[p] = l;
        nl += l;
    }
    if (threadIdx.x == 0) *nlive = nl;
}

// symmp_live_kernel with every pair taken as live, whatever its solver's state (a product that scores every column)
__global__ __launch_bounds__(64) void symmp_all_live_kernel(const int *__restrict__ pairs, int m, int ncls, int kpad,
                                                           int *__restrict__ plive, int *__restrict__ ccnt, int *__restrict__ cslot) {
    for (int c = threadIdx.x; c < ncls; c += 64) {
        int k = 0;
        for (int p = 0; p < m; ++p)
            if (pairs[2 * p] == c || pairs[2 * p + 1] == c) cslot[c * kpad + k++] = p;
        ccnt[c] = k;
    }
    for (int p = threadIdx.x; p < m; p += 64) plive[p] = 1;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------

void bq_pairs_plan_destroy(bq_pairs_plan *pl) {
    if (pl == nullptr) return;
    delete pl;
}

int64_t bq_pairs_slab_len(const bq_pairs_plan *pl) { return pl->slab_len; }

const int *bq_pairs_plan_tiles(const bq_pairs_plan *pl) { return pl->dct; }
const int *bq_pairs_plan_pairs(const bq_pairs_plan *pl) { return pl->dpairs; }
int bq_pairs_plan_ncls(const bq_pairs_plan *pl) { return pl->ncls; }
const int *bq_pairs_plan_host_tiles(const bq_pairs_plan *pl) { return pl->ct.data(); }
const int *bq_pairs_plan_host_pairs(const bq_pairs_plan *pl) { return pl->pairs.data(); }

// every pair live: the plan's start state (and what a one-off product takes)
static int plan_all_live(bq_pairs_plan *pl, hipStream_t st) {
    std::vector<int> live(pl->m, 1), cnt(pl->ncls, 0), slot((size_t)pl->ncls * pl->kpad, 0);
    for (int p = 0; p < pl->m; ++p)
        for (int e = 0; e < 2; ++e) {
            const int c = pl->pairs[2 * p + e];
            slot[(size_t)c * pl->kpad + cnt[c]++] = p;
        }
    BQ_HIP(hipMemcpyAsync(pl->plive, live.data(), sizeof(int) * live.size(), hipMemcpyHostToDevice, st));
    BQ_HIP(hipMemcpyAsync(pl->ccnt, cnt.data(), sizeof(int) * cnt.size(), hipMemcpyHostToDevice, st));
    BQ_HIP(hipMemcpyAsync(pl->cslot, slot.data(), sizeof(int) * slot.size(), hipMemcpyHostToDevice, st));
    return hipStreamSynchronize(st) == hipSuccess ? BQ_OK : BQ_ERR_HIP;   // the host vectors go out of scope
}

int bq_pairs_plan_create(bq_problem *p, int ncls, const int *cls_tiles, int m, const int *pairs, bq_pairs_plan **out) {
    BQ_ARG(p && out, "NULL argument");
    BQ_TRY(check_pairs(p->nb, ncls, cls_tiles, m, pairs));
    std::vector<pitem> single, diag;
    std::vector<int> cnt;
    build_lists(ncls, cls_tiles, m, pairs, single, diag, cnt);
    bq_pairs_plan *pl = new bq_pairs_plan();
    pl->ncls = ncls;
    pl->m = m;
    pl->nb = p->nb;
    pl->ct.assign(cls_tiles, cls_tiles + ncls + 1);
    pl->pairs.assign(pairs, pairs + 2 * m);
    const int cmax = *std::max_element(cnt.begin(), cnt.end());
    pl->nch = (cmax + CK - 1) / CK;
    pl->kpad = pl->nch * CK;
    pl->nsingle = (int64_t)single.size();
    pl->ndiag = (int64_t)diag.size();
    std::vector<pinfo> info(m);
    int64_t base = 0;
    for (int q = 0; q < m; ++q) {
        const int a = pairs[2 * q], b = pairs[2 * q + 1];
        pinfo &pi = info[q];
        pi.base = base;
        pi.na = cls_tiles[a + 1] - cls_tiles[a];
        pi.L = pi.na + cls_tiles[b + 1] - cls_tiles[b];
        pi.ns = (pi.na + JG - 1) / JG;
        pi.a0 = cls_tiles[a];
        pi.b0 = cls_tiles[b];
        base += (int64_t)pi.L * pi.L * ST;
        pl->lmax = std::max(pl->lmax, pi.L);
    }
    pl->slab_len = base;
    pl->single = pl->mem.dev<pitem>(std::max<size_t>(1, single.size()));
    pl->diag = pl->mem.dev<pitem>(std::max<size_t>(1, diag.size()));
    pl->info = pl->mem.dev<pinfo>(m);
    pl->dct = pl->mem.dev<int>(ncls + 1);
    pl->dpairs = pl->mem.dev<int>(2 * m);
    pl->plive = pl->mem.dev<int>(m);
    pl->ccnt = pl->mem.dev<int>(ncls);
    pl->cslot = pl->mem.dev<int>((size_t)ncls * pl->kpad);
    hipError_t e = pl->mem.error();
    hipStream_t st = p->ctx->stream;
    if (e == hipSuccess && !single.empty()) e = hipMemcpyAsync(pl->single, single.data(), sizeof(pitem) * single.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && !diag.empty()) e = hipMemcpyAsync(pl->diag, diag.data(), sizeof(pitem) * diag.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(pl->info, info.data(), sizeof(pinfo) * m, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(pl->dct, cls_tiles, sizeof(int) * (ncls + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(pl->dpairs, pairs, sizeof(int) * 2 * m, hipMemcpyHostToDevice, st);
    int rc = BQ_OK;
    if (e != hipSuccess) {
        bq_set_error("pair plan setup failed: %s", hipGetErrorString(e));
        rc = e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
    }
    if (rc == BQ_OK) rc = plan_all_live(pl, st);
    if (rc != BQ_OK) {
        (void)hipStreamSynchronize(st);
        bq_pairs_plan_destroy(pl);
        return rc;
    }
    *out = pl;
    return BQ_OK;
}

int bq_launch_pairs_live(const bq_pairs_plan *pl, bq_scal *const *scs, int *nlive, hipStream_t st) {
    symmp_live_kernel<<<1, 64, 0, st>>>(scs, pl->dpairs, pl->m, pl->ncls, pl->kpad, pl->plive, pl->ccnt, pl->cslot, nlive);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

int bq_launch_pairs_all_live(const bq_pairs_plan *pl, hipStream_t st) {
    symmp_all_live_kernel<<<1, 64, 0, st>>>(pl->dpairs, pl->m, pl->ncls, pl->kpad, pl->plive, pl->ccnt, pl->cslot);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

int bq_launch_symmp(bq_problem *p, const bq_pairs_plan *pl, bool add_one, const double *W, int64_t ldw, double *slab, double *out) {
    BQ_ARG(p->symmetric && !p->streamed && p->ctx->world == 1, "the routed product needs a resident packed panel on one rank");
    BQ_ARG(ldw >= p->nb * ST && pl->nb == p->nb, "column stride shorter than the panel, or a plan of another panel");
    hipStream_t st = p->ctx->stream;
    bq_panel_dispatch(p, add_one, [&](auto pv, auto one) {
        using T = bq_pelem<decltype(pv)>;
        constexpr bool ADD_ONE = decltype(one)::value;
        // fp32 tiles are half as wide in bytes: 8 rows per step keep the same bytes in flight per lane (bq_symv.hip); fp64 and the
        // compact layout (its decode spills at 8): 4
        constexpr int SR = std::is_same<T, float>::value ? 8 : 4;
        if (pl->nsingle > 0)
            symmp_single_kernel<T, ADD_ONE, SR><<<(unsigned)pl->nsingle, 256, 0, st>>>(pv, pl->single, pl->info, pl->plive, W, ldw, slab);
        if (pl->ndiag > 0)
            symmp_diag_kernel<T, ADD_ONE><<<dim3((unsigned)pl->ndiag, (unsigned)pl->nch), 256, 0, st>>>(
                pv, pl->diag, pl->info, pl->dpairs, pl->dct, pl->ccnt, pl->cslot, pl->kpad, W, ldw, slab);
    });
    symmp_reduce_kernel<<<dim3((unsigned)pl->lmax, (unsigned)pl->m), 1024, 0, st>>>(slab, pl->info, pl->plive, out, ldw);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------------------

extern "C" int bq_pairs_work_list(int64_t nb, int ncls, const int *cls_tiles, int m, const int *pairs, int *items, int64_t cap,
                                  int64_t *count) {
    BQ_ARG(count != nullptr, "NULL argument");
    BQ_TRY(check_pairs(nb, ncls, cls_tiles, m, pairs));
    std::vector<pitem> single, diag;
    std::vector<int> cnt;
    build_lists(ncls, cls_tiles, m, pairs, single, diag, cnt);
    *count = (int64_t)(single.size() + diag.size());
    if (items == nullptr) return BQ_OK;
    BQ_ARG(cap >= *count, "items capacity is smaller than the work list");
    int64_t i = 0;
    for (int kind = 0; kind < 2; ++kind)
        for (const pitem &it : kind == 0 ? single : diag) {
            int *r = items + 5 * i++;
            r[0] = kind;
            r[1] = it.I;
            r[2] = it.J0;
            r[3] = it.nj;
            r[4] = it.id;
        }
    return BQ_OK;
}

extern "C" int bq_pairs_slab_bytes(int64_t nb, int ncls, const int *cls_tiles, int m, const int *pairs, int64_t *bytes) {
    BQ_ARG(bytes != nullptr, "NULL argument");
    BQ_TRY(check_pairs(nb, ncls, cls_tiles, m, pairs));
    *bytes = (int64_t)sizeof(double) * slab_len(cls_tiles, m, pairs);
    return BQ_OK;
}

extern "C" int bq_problem_gram_matmat_pairs(bq_problem *p, int ncls, const int *cls_tiles, int m, const int *pairs, const double *W,
                                            double *out) {
    BQ_ARG(p && W && out, "NULL argument");
    BQ_ARG(p->kernel >= 0, "not a kernel-structured problem");
    BQ_TRY(bq_need_resident_panel(p, "the routed product"));
    BQ_HIP(hipSetDevice(p->ctx->device));
    bq_pairs_plan *pl = nullptr;
    BQ_TRY(bq_pairs_plan_create(p, ncls, cls_tiles, m, pairs, &pl));
    // OUT is zero-filled first: the rows outside a pair's classes are never written and must read exact 0.0
    struct call { bq_problem *p; const bq_pairs_plan *pl; } cl{p, pl};
    const int rc = bq_product_once(
        p, "gram_matmat_pairs", m, m, pl->slab_len, true, W, out,
        [](void *arg, const double *dW, int64_t ldw, double *slab, double *dO, const int *) {
            const call *c = (const call *)arg;
            return bq_launch_symmp(c->p, c->pl, false, dW, ldw, slab, dO);
        },
        &cl);
    bq_pairs_plan_destroy(pl);
    return rc;
}
