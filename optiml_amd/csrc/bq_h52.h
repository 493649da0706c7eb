// The Hessian image of a compact RBF panel: h = fl(K + 1) in 6.5 bytes per element (host + device; free of HIP for a host compiler, so
// that tests/c/h52_check.cpp checks the same functions).
//
// The rank-one duals (SVC / SVR with the regularised intercept: bq_problem::add_one) multiply by K + 1, and a compact panel (bq_c7.h)
// holds K in {0} u [2^-14, 1] — 2^-15 as the bound that encode enforces —, so h lies in {1.0} u [1 + 2^-15, 2.0]: the exponent is that of
// 1.0 except for h = 2.0 (K = 1: the diagonal, duplicate rows of X, K = 1 - 2^-53), and the value is its 52 mantissa bits.
//   code 0              -> 1.0   (the zero pad of the panel: 0.0 + 1.0; a memset image decodes to 1.0 everywhere)
//   code 1              -> 2.0   (the escape: 1 + 2^-52 cannot occur, since K >= 2^-15 would have to be 2^-52)
//   any other code m    -> the fp64 value with the high word 0x3FF00000 | m >> 32 and the low word m
// encode refuses every h outside {1.0} u [1 + 2^-15, 2.0].  Each encodable h comes back bit for bit.
//
// Three planes over one allocation of 6.5 x elems bytes, elems the panel's (a multiple of 65 536): `lo` bits 0-31 (4 B per element), then
// `mid` bits 32-47 (2 B), then `nib` bits 48-51 (4 bits; the element at the even position in the low nibble of its byte).  Strip, row
// and tile offsets are those of bq_sym_addr.  Inside one row of one tile — an aligned run of 256 positions — the elements lie in LANE
// ORDER: position 4 l + {0, 1, 2, 3} holds the columns 2 l, 2 l + 1, 128 + 2 l, 128 + 2 l + 1 that lane l of the tile product owns
// (tile_ld, bq_symv_tile.h), so a lane reads 16 + 8 + 2 contiguous bytes per row and tile and a wave 1 024 + 512 + 128.
#pragma once
#include <cstdint>

#include "bq_sym_layout.h"

struct bq_h52 {};   // element tag of the image: an instantiation of symv_tiles_kernel, of nothing else

constexpr uint64_t BQ_H52_ONE = 0x3FF0000000000000ull, BQ_H52_TWO = 0x4000000000000000ull;
constexpr uint64_t BQ_H52_MIN_MANT = 1ull << 37;   // 2^-15 in the mantissa of a value in [1, 2)

// the 52-bit code of the fp64 bit pattern `b`; *bad is set (never cleared) when b is outside the domain, and the code is then 0
BQ_HD inline uint64_t bq_h52_encode(uint64_t b, bool *bad) {
    if (b == BQ_H52_ONE) return 0;
    if (b == BQ_H52_TWO) return 1;
    const uint64_t m = b & 0x000FFFFFFFFFFFFFull;
    if ((b >> 52) == 0x3FF && m >= BQ_H52_MIN_MANT) return m;
    *bad = true;
    return 0;
}
// the fp64 bit pattern of a code given as its planes' fields: m20 = nib << 16 | mid
BQ_HD inline uint32_t bq_h52_hi(uint32_t lo, uint32_t m20) { return (m20 == 0 && lo == 1) ? 0x40000000u : (0x3FF00000u | m20); }
BQ_HD inline uint32_t bq_h52_lo(uint32_t lo, uint32_t m20) { return (m20 == 0 && lo == 1) ? 0u : lo; }
BQ_HD inline uint64_t bq_h52_bits(uint32_t lo, uint32_t mid, uint32_t nib) {
    const uint32_t m20 = (nib << 16) | mid;
    return ((uint64_t)bq_h52_hi(lo, m20) << 32) | bq_h52_lo(lo, m20);
}

constexpr int64_t BQ_H52_ROW = 256;   // one row of one tile: the unit of the lane order (== BQ_SYM_TILE)
// position inside a tile row of column c, and the column at position q
BQ_HD inline int bq_h52_pos(int c) { return 4 * ((c & 127) >> 1) + 2 * (c >> 7) + (c & 1); }
BQ_HD inline int bq_h52_col(int q) { return 2 * (q >> 2) + 128 * ((q >> 1) & 1) + (q & 1); }
// image position of the panel element at packed index `a` (bq_sym_addr: every aligned run of 256 indices is one row of one tile)
BQ_HD inline int64_t bq_h52_addr(int64_t a) { return (a & ~(BQ_H52_ROW - 1)) + bq_h52_pos((int)(a & (BQ_H52_ROW - 1))); }
BQ_HD inline int64_t bq_h52_bytes(int64_t elems) { return 6 * elems + elems / 2; }

// read side: a "pointer" to position k (even) of every plane; + as for the panel views
struct bq_h52p {
    const uint32_t *lo;
    const uint16_t *mid;
    const uint8_t *nib;
    BQ_HD inline bq_h52p operator+(int64_t k) const { return {lo + k, mid + k, nib + (k >> 1)}; }
};
static inline bq_h52p bq_h52_view(const void *base, int64_t elems) {
    const unsigned char *b = (const unsigned char *)base;
    return {(const uint32_t *)b, (const uint16_t *)(b + 4 * elems), (const uint8_t *)(b + 6 * elems)};
}
// host-side element access (the checks and nothing else)
static inline void bq_h52_put(void *base, int64_t elems, int64_t pos, uint64_t code) {
    unsigned char *b = (unsigned char *)base;
    ((uint32_t *)b)[pos] = (uint32_t)code;
    ((uint16_t *)(b + 4 * elems))[pos] = (uint16_t)(code >> 32);
    unsigned char &n = b[6 * elems + (pos >> 1)];
    const unsigned v = (unsigned)(code >> 48) & 0xFu;
    n = (pos & 1) ? (unsigned char)((n & 0x0Fu) | (v << 4)) : (unsigned char)((n & 0xF0u) | v);
}
static inline uint64_t bq_h52_get(const void *base, int64_t elems, int64_t pos) {
    const bq_h52p v = bq_h52_view(base, elems);
    return bq_h52_bits(v.lo[pos], v.mid[pos], (v.nib[pos >> 1] >> ((pos & 1) * 4)) & 0xFu);
}
