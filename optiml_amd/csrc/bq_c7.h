// The compact fp64 panel layout: an RBF Gram entry lies in (0, 1], and every fp64 value in [2^-15, 2) has the top byte 0x3F
// (sign 0, the upper seven exponent bits).  An eligible panel (bq_c7_eligible) therefore stores each element in 7 bytes, in three
// planes over the packed lower-triangle index of bq_sym_addr (strip after strip: bq_sym_layout.h; one index for all three planes): `lo` bits 0-31 (4 B), `mid` bits 32-47 (2 B), `top` bits 48-55 (1 B),
// in one allocation of elems x 7 bytes (lo plane, then mid, then top).  Columns keep their natural order within a row, so an
// adjacent column pair is 8 + 4 + 2 naturally aligned bytes and one element 4 + 2 + 1.
// Zero code: all 56 stored bits zero decode to +0.0 (the memset panel and the zero pad of the ragged last tile row / column), so the
// pattern 0x3F00000000000000 (2^-15 exactly) cannot be stored.  Every stored element comes back bit for bit.
#pragma once
#include <cmath>
#include <type_traits>
#include <utility>

#include "bq_common.h"

struct bq_c7 {};   // element tag of the compact layout: the third instantiation of the T-templated panel readers

__host__ __device__ inline bool bq_c7_encodable(uint64_t b) {
    return b == 0 || ((b >> 56) == 0x3F && (b & 0x00FFFFFFFFFFFFFFull) != 0);
}
// the 24 bits above `lo`: (top << 16) | mid -> the high word of the fp64 value
__host__ __device__ inline uint32_t bq_c7_hi(uint32_t lo, uint32_t m24) { return (m24 | lo) == 0 ? 0u : (0x3F000000u | m24); }
__host__ __device__ inline uint64_t bq_c7_bits(uint32_t lo, uint32_t mid, uint32_t top) {
    return ((uint64_t)bq_c7_hi(lo, (top << 16) | mid) << 32) | lo;
}

// Exactness rule of a compact RBF panel: K_ij = exp(-gamma D_ij) with D_ij <= (|x_i| + |x_j|)^2 <= 4 max |x|^2, so
// exp(-gamma 4 max |x|^2) >= 2^-14 keeps every element in [2^-14, 1] (a factor of 2 of margin against the rounding of D).
static inline bool bq_c7_eligible(double gamma, double max_sq_norm) {
    return gamma >= 0.0 && std::isfinite(max_sq_norm) && std::exp(-gamma * 4.0 * max_sq_norm) >= 0x1p-14;
}

// read side: a "pointer" to element k of every plane; + and [] as for a const double *
struct bq_c7p {
    const uint32_t *lo;
    const uint16_t *mid;
    const uint8_t *top;
    __host__ __device__ __forceinline__ bq_c7p operator+(int64_t k) const { return {lo + k, mid + k, top + k}; }
    __device__ __forceinline__ double operator[](int64_t k) const {
        const uint32_t l = lo[k];
        return __hiloint2double((int)bq_c7_hi(l, ((uint32_t)top[k] << 16) | mid[k]), (int)l);
    }
    // elements k, k + 1 (k even): one 8-byte, one 4-byte and one 2-byte non-temporal load
    typedef double d2 __attribute__((ext_vector_type(2)));
    __device__ __forceinline__ d2 pair(int64_t k) const {
        typedef unsigned int u2_t __attribute__((ext_vector_type(2)));
        const u2_t l = __builtin_nontemporal_load(reinterpret_cast<const u2_t *>(lo + k));
        const uint32_t m = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(mid + k));
        const uint32_t t = __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(top + k));
        d2 v;
        v.x = __hiloint2double((int)bq_c7_hi(l.x, ((t & 0xFFu) << 16) | (m & 0xFFFFu)), (int)l.x);
        v.y = __hiloint2double((int)bq_c7_hi(l.y, ((t >> 8) << 16) | (m >> 16)), (int)l.y);
        return v;
    }
};
static inline bq_c7p bq_c7_view(const void *base, int64_t elems) {
    const unsigned char *b = (const unsigned char *)base;
    return {(const uint32_t *)b, (const uint16_t *)(b + 4 * elems), (const uint8_t *)(b + 6 * elems)};
}

// write side (the Gram epilogue): an element that cannot be stored raises *bad (a plain vector store) and is written as it encodes
struct bq_c7w {
    uint32_t *lo;
    uint16_t *mid;
    uint8_t *top;
    int *bad;
    __host__ __device__ __forceinline__ bq_c7w operator+(int64_t k) const { return {lo + k, mid + k, top + k, bad}; }
};
static inline bq_c7w bq_c7_wview(void *base, int64_t elems, int *bad) {
    unsigned char *b = (unsigned char *)base;
    return {(uint32_t *)b, (uint16_t *)(b + 4 * elems), (uint8_t *)(b + 6 * elems), bad};
}

// the panel "pointer" of a T-templated reader: const T * for fp64 / fp32, the plane view for the compact layout
// (bq_pptr: kernel parameters, restrict as they were; bq_pview: struct members)
template <typename T> struct bq_pan {
    typedef const T *__restrict__ ptr;
    typedef const T *view;
};
template <> struct bq_pan<bq_c7> {
    typedef bq_c7p ptr;
    typedef bq_c7p view;
};
template <typename T> using bq_pptr = typename bq_pan<T>::ptr;
template <typename T> using bq_pview = typename bq_pan<T>::view;

// a problem's resident panel as a T reader takes it
template <typename T> static inline bq_pview<T> bq_panel_as(const bq_problem *p) { return (const T *)p->panel; }
template <> inline bq_c7p bq_panel_as<bq_c7>(const bq_problem *p) { return bq_c7_view(p->panel, p->panel_elems); }

// the element type T of a typed panel view, and the storage dispatch of the T-templated launchers: f(the panel's typed view,
// std::bool_constant<add_one>) — `f` is a generic lambda that launches kernel<bq_pelem<decltype(view)>, decltype(one)::value>
template <typename V> struct bq_view_elem { typedef std::remove_cv_t<std::remove_pointer_t<V>> type; };
template <> struct bq_view_elem<bq_c7p> { typedef bq_c7 type; };
template <typename V> using bq_pelem = typename bq_view_elem<V>::type;

template <typename F> static inline void bq_panel_dispatch(const bq_panel_ref &panel, bool add_one, F &&f) {
    auto typed = [&](auto pv) {
        if (add_one) f(pv, std::true_type{});
        else f(pv, std::false_type{});
    };
    if (panel.storage == BQ_F64C) typed(bq_c7_view(panel.base, panel.elems));
    else if (panel.storage == BQ_F64) typed((const double *)panel.base);
    else typed((const float *)panel.base);
}
template <typename F> static inline void bq_panel_dispatch(const bq_problem *p, bool add_one, F &&f) {
    bq_panel_dispatch(bq_problem_panel(p), add_one, std::forward<F>(f));
}
