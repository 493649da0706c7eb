// Pieces shared by the symmetric panel products (bq_symv.hip: one column; bq_symm.hip, bq_symmw.hip: several; bq_symmp.hip: one per
// class pair): the 16-byte tile loads, the linear strip index of a tile row and the fixed-order walk of a slab column.
#pragma once
#include "bq_c7.h"
#include "bq_common.h"
#include "bq_h52.h"

typedef double d2_t __attribute__((ext_vector_type(2)));

constexpr int ST = 256;   // tile edge (== BQ_SYM_TILE)

typedef float f4_t __attribute__((ext_vector_type(4)));

// One 16-byte non-temporal load per lane and row.  fp64: a lane owns columns {2l, 2l+1} and {128+2l, 128+2l+1} of a tile
// (two loads); fp32: columns {4l .. 4l+3} (one float4 load).  c0 / c1 are the first columns of the two pairs.
template <typename T> struct tile_ld;
template <> struct tile_ld<double> {
    static __device__ __forceinline__ int c0(int lane) { return 2 * lane; }
    static __device__ __forceinline__ int c1(int lane) { return 128 + 2 * lane; }
    static __device__ __forceinline__ void get(const double *row, int lane, d2_t &a, d2_t &b) {
        a = __builtin_nontemporal_load(reinterpret_cast<const d2_t *>(row + 2 * lane));
        b = __builtin_nontemporal_load(reinterpret_cast<const d2_t *>(row + 128 + 2 * lane));
    }
};
template <> struct tile_ld<bq_c7> {   // the compact layout (bq_c7.h): per pair one 8-, one 4- and one 2-byte load, same columns as fp64
    static __device__ __forceinline__ int c0(int lane) { return 2 * lane; }
    static __device__ __forceinline__ int c1(int lane) { return 128 + 2 * lane; }
    static __device__ __forceinline__ void get(const bq_c7p &row, int lane, d2_t &a, d2_t &b) {
        a = row.pair(2 * lane);
        b = row.pair(128 + 2 * lane);
    }
};
// The Hessian image (bq_h52.h): a tile row lies in lane order, so the lane's four columns are one 16-byte, one 8-byte and one 2-byte
// load — three requests per row and tile where the compact panel takes six.  The values are fl(K + 1): the kernel adds nothing.
template <> struct bq_pan<bq_h52> {
    typedef bq_h52p ptr;
    typedef bq_h52p view;
};
template <> struct tile_ld<bq_h52> {
    static __device__ __forceinline__ int c0(int lane) { return 2 * lane; }
    static __device__ __forceinline__ int c1(int lane) { return 128 + 2 * lane; }
    // the loads only: the 7 loaded words travel in a / b as they came (a: lo of the four columns, b.x: their mid, b.y: their nib) and
    // tile_post<bq_h52>::decode turns them into the values — so that the kernel can keep every load of a step ahead of the first decode.
    // Each plane is loaded AS the type it travels in: repacked from an integer vector, the 16-byte load came out twice in the ISA (a
    // dwordx4 and a dwordx2 of the same address).
    static __device__ __forceinline__ void get(const bq_h52p &row, int lane, d2_t &a, d2_t &b) {
        a = __builtin_nontemporal_load(reinterpret_cast<const d2_t *>(row.lo + 4 * lane));
        b.x = __builtin_nontemporal_load(reinterpret_cast<const double *>(row.mid + 4 * lane));
        b.y = __hiloint2double(0, (int)(uint32_t)__builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(row.nib + 2 * lane)));
    }
};
template <> struct tile_ld<float> {
    static __device__ __forceinline__ int c0(int lane) { return 4 * lane; }
    static __device__ __forceinline__ int c1(int lane) { return 4 * lane + 2; }
    static __device__ __forceinline__ void get(const float *row, int lane, d2_t &a, d2_t &b) {
        const f4_t v = __builtin_nontemporal_load(reinterpret_cast<const f4_t *>(row + 4 * lane));
        a = (d2_t){(double)v.x, (double)v.y};
        b = (d2_t){(double)v.z, (double)v.w};
    }
};

// What a layout does between the loads of a step and its FMAs; nothing for the layouts whose tile_ld::get returns values.
template <typename T> struct tile_post {
    static __device__ __forceinline__ void issued() {}
    static __device__ __forceinline__ void decode(d2_t &, d2_t &) {}
};
// The image: left to itself the compiler sinks the loads of the later rows of a step below the waits and decodes of the earlier
// ones (at most six loads in flight, the step's latency paid row after row: 6.15 - 6.33 ms at the headline where the compact panel takes
// 5.47 - 5.60, profiles/hessian_image/headline_ab_first_schedule.json) — the scheduling barrier keeps all of a step's loads ahead.
template <> struct tile_post<bq_h52> {
    static __device__ __forceinline__ void issued() { __builtin_amdgcn_sched_barrier(0); }
    // bq_h52_bits with its two-sided escape test folded into one compare: z = m20 | (lo ^ 1) is 0 for the code 1 alone
    static __device__ __forceinline__ double val(uint32_t lo, uint32_t m20) {
        const uint32_t z = m20 | (lo ^ 1u);
        return __hiloint2double((int)(z ? (0x3FF00000u | m20) : 0x40000000u), (int)(z ? lo : 0u));
    }
    static __device__ __forceinline__ void decode(d2_t &a, d2_t &b) {
        const uint32_t l0 = (uint32_t)__double2loint(a.x), l1 = (uint32_t)__double2hiint(a.x);
        const uint32_t l2 = (uint32_t)__double2loint(a.y), l3 = (uint32_t)__double2hiint(a.y);
        const uint32_t m0 = (uint32_t)__double2loint(b.x), m1 = (uint32_t)__double2hiint(b.x), t = (uint32_t)__double2loint(b.y);
        a.x = val(l0, ((t & 0xFu) << 16) | (m0 & 0xFFFFu));
        a.y = val(l1, ((t & 0xF0u) << 12) | (m0 >> 16));
        b.x = val(l2, ((t & 0xF00u) << 8) | (m1 & 0xFFFFu));
        b.y = val(l3, ((t & 0xF000u) << 4) | (m1 >> 16));
    }
};

// strips of tile row I: g = 0 .. I / JG ; linear index over tile rows [I0, I1)
template <int JG>
__device__ __host__ __forceinline__ int64_t strips_before(int64_t I) {  // sum_{i < I} (i / JG + 1)
    const int64_t qq = I / JG, rr = I % JG;
    return JG * qq * (qq + 1) / 2 + rr * (qq + 1);
}

// The fixed-order walk of a slab column: entries first, first + 4, ... < count of `base` (stride doubles apart) are added to two
// chains (s0: entries k, k + 8, ...; s1: k + 4, k + 12, ...), each in its own order — but the LOADS of four turns are issued
// together (round 5): written as one load per turn the loop was a chain of L2 round trips (~11 of them at nb = 79, ~50 at nb = 391:
// most of the reduce kernel's 7 us on short grids); the association, and with it every bit, is what it was.
__device__ __forceinline__ void slab_walk(const double *base, int64_t first, int64_t count, int64_t stride, double &s0, double &s1) {
    int64_t k = first;
    for (; k + 28 < count; k += 32) {   // four turns of both chains: all eight entries exist
        const double a0 = base[(k) * stride], b0 = base[(k + 4) * stride], a1 = base[(k + 8) * stride], b1 = base[(k + 12) * stride];
        const double a2 = base[(k + 16) * stride], b2 = base[(k + 20) * stride], a3 = base[(k + 24) * stride], b3 = base[(k + 28) * stride];
        s0 += a0;
        s1 += b0;
        s0 += a1;
        s1 += b1;
        s0 += a2;
        s1 += b2;
        s0 += a3;
        s1 += b3;
    }
    for (; k < count; k += 8) {
        s0 += base[k * stride];
        if (k + 4 < count) s1 += base[(k + 4) * stride];
    }
}

// Partial sum of output block a over the slab entries S[a][b] that the tile rows [c0, c1) produced, b ascending:
//   row parts live at b = first tile of a strip (b % JG == 0, b <= a) when tile row a lies in [c0, c1),
//   col parts at every b > a inside [c0, c1).
// 1024 threads: thread (r, q) sums every 4th entry of that fixed entry list (slab_walk's two chains); the four partial sums are
// combined in the fixed order q = 0..3.  Every thread returns the combined value.
template <int JG>
__device__ __forceinline__ double seg_thread_sum(const double *__restrict__ p, int64_t a, int64_t c0, int64_t c1, int q) {
    double s0 = 0.0, s1 = 0.0;
    int64_t e = 0;   // running index over the entry list: row parts (b = 0, JG, 2JG, ... <= a) then col parts (b > a)
    if (a >= c0 && a < c1) {
        const int64_t nrow = a / JG + 1;
        slab_walk(p, q, nrow, (int64_t)JG * ST, s0, s1);
        e = nrow;
    }
    const int64_t bs = (a + 1 > c0) ? a + 1 : c0;
    const int64_t ncol = c1 > bs ? c1 - bs : 0;
    // keep the q-assignment a function of the position in the whole list (row parts first)
    const int64_t shift = (4 - (e & 3)) & 3;
    slab_walk(p + bs * ST, (q + shift) & 3, ncol, ST, s0, s1);
    return s0 + s1;   // this thread's share (every 4th entry, q = its phase) of the segment's entry list
}
