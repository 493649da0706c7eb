// The address function of the packed symmetric panel layout (included by bq_common.h; plain C++ so that a host program can check it).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define BQ_HD __host__ __device__
#else
#define BQ_HD
#endif

constexpr int64_t BQ_SYM_TILE = 256;
// Packed layout of a symmetric (kernel-built) panel: tile row I (256 rows) keeps only its columns [0, (I+1)*256); tile rows
// are concatenated (tile row I starts at bq_sym_off(I)).  Inside a tile row the STRIPS — BQ_SYM_STRIP consecutive tiles, the
// work item of the strip kernels — lie one after another, each its own row-major 256 x W block, W = bq_sym_strip_w: 2048
// elements, or what is left of the row for its last strip.  A strip is one contiguous run (4 MiB of fp64), its rows stay
// 16-byte aligned and W is a multiple of 256.  Element (i, j), j's tile <= i's tile, of a panel whose first stored tile
// row is I0, lives at bq_sym_addr; a row is contiguous only within a strip.
constexpr int64_t BQ_SYM_STRIP = 8;   // tiles per strip: every strip kernel static_asserts its JG against it
constexpr int64_t BQ_SYM_STRIP_COLS = BQ_SYM_STRIP * BQ_SYM_TILE;
BQ_HD inline int64_t bq_sym_off(int64_t I) { return BQ_SYM_TILE * BQ_SYM_TILE * (I * (I + 1) / 2); }
BQ_HD inline int64_t bq_sym_cols(int64_t I) { return (I + 1) * BQ_SYM_TILE; }   // stored columns of tile row I
BQ_HD inline int64_t bq_sym_strip_w(int64_t I, int64_t g) {   // row pitch of strip g of tile row I
    const int64_t rest = bq_sym_cols(I) - g * BQ_SYM_STRIP_COLS;
    return rest < BQ_SYM_STRIP_COLS ? rest : BQ_SYM_STRIP_COLS;
}
BQ_HD inline int64_t bq_sym_strip_off(int64_t I, int64_t g) {   // first element of strip g of tile row I
    return bq_sym_off(I) + g * (BQ_SYM_TILE * BQ_SYM_STRIP_COLS);
}
BQ_HD inline int64_t bq_sym_addr(int64_t i, int64_t j, int64_t I0) {
    const int64_t I = i / BQ_SYM_TILE, g = j / BQ_SYM_STRIP_COLS;
    return bq_sym_strip_off(I, g) - bq_sym_off(I0) + (i - I * BQ_SYM_TILE) * bq_sym_strip_w(I, g) + (j - g * BQ_SYM_STRIP_COLS);
}
