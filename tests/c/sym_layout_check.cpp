// Host check of the packed symmetric panel's address function (optiml_amd/csrc/bq_sym_layout.h), the one every reader and writer
// of the panel goes through.  For nb = 1 .. 40 tile rows: (I, r, c <= the row's width) -> address is a bijection onto [0, elems);
// a strip is one contiguous run whose rows are 16-byte aligned for fp64 and fp32 and 2-element aligned for the compact pairs; the
// share contexts' origin (I0 > 0) only shifts the map.  Built by tests/test_sym_layout_host.py (with ASan + UBSan where available).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bq_sym_layout.h"

static int fails = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (++fails <= 20) {              \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);     \
                std::printf("\n");            \
            }                                 \
        }                                     \
    } while (0)

int main() {
    const int64_t T = BQ_SYM_TILE, SC = BQ_SYM_STRIP_COLS;
    static_assert(BQ_SYM_STRIP == 8, "DESIGN: a strip is 8 tiles");
    // The map of a panel of nb tile rows is the map of tile rows I < nb (the address function does not take nb): the tile rows are
    // walked once, and after tile row nb - 1 the addresses seen so far must be exactly [0, elems(nb)).
    const int64_t NB = 40;
    std::vector<unsigned char> seen((size_t)bq_sym_off(NB), 0);
    int64_t hit = 0;
    for (int64_t nb = 1; nb <= NB; ++nb) {
        const int64_t elems = bq_sym_off(nb);
        CHECK(elems == T * T * nb * (nb + 1) / 2, "nb=%lld", (long long)nb);
        {
            const int64_t I = nb - 1;
            const int64_t cols = bq_sym_cols(I);
            CHECK(cols == (I + 1) * T, "I=%lld", (long long)I);
            int64_t wsum = 0;
            for (int64_t g = 0; g * SC < cols; ++g) {
                const int64_t W = bq_sym_strip_w(I, g);
                wsum += W;
                CHECK(W > 0 && W <= SC && W % T == 0, "I=%lld g=%lld W=%lld", (long long)I, (long long)g, (long long)W);
                CHECK(W == SC || (g + 1) * SC >= cols, "only the last strip is narrow: I=%lld g=%lld", (long long)I, (long long)g);
                // the strip is the contiguous run [strip_off, strip_off + 256 W) and follows the one before it
                const int64_t s0 = bq_sym_strip_off(I, g);
                CHECK(s0 == bq_sym_addr(I * T, g * SC, 0), "strip start I=%lld g=%lld", (long long)I, (long long)g);
                CHECK(s0 == bq_sym_off(I) + g * T * SC, "strips follow one another I=%lld g=%lld", (long long)I, (long long)g);
                CHECK(bq_sym_addr(I * T + T - 1, g * SC + W - 1, 0) == s0 + T * W - 1, "strip end I=%lld g=%lld", (long long)I, (long long)g);
                for (int64_t r = 0; r < T; ++r) {
                    const int64_t row0 = bq_sym_addr(I * T + r, g * SC, 0);
                    CHECK(row0 == s0 + r * W, "row-major in the strip");
                    // 16 bytes: 2 fp64 or 4 fp32 elements; compact pairs: 2 elements (8 + 4 + 2 bytes, each naturally aligned)
                    CHECK((row0 * 8) % 16 == 0 && (row0 * 4) % 16 == 0 && row0 % 2 == 0, "row alignment I=%lld g=%lld r=%lld", (long long)I,
                          (long long)g, (long long)r);
                    CHECK((W * 8) % 2048 == 0 && (W * 4) % 1024 == 0, "pitch");
                }
            }
            CHECK(wsum == cols, "strip widths cover the row: I=%lld", (long long)I);
            for (int64_t r = 0; r < T; ++r)
                for (int64_t c = 0; c < cols; ++c) {
                    const int64_t a = bq_sym_addr(I * T + r, c, 0);
                    if (a < 0 || a >= elems) {
                        CHECK(false, "out of range nb=%lld I=%lld r=%lld c=%lld a=%lld", (long long)nb, (long long)I, (long long)r, (long long)c,
                              (long long)a);
                        continue;
                    }
                    CHECK(a >= bq_sym_off(I) && a < bq_sym_off(I + 1), "inside its tile row");
                    CHECK(!seen[(size_t)a], "twice: nb=%lld I=%lld r=%lld c=%lld", (long long)nb, (long long)I, (long long)r, (long long)c);
                    seen[(size_t)a] = 1;
                    ++hit;
                    if (c + 1 < cols && (c + 1) % SC != 0) CHECK(bq_sym_addr(I * T + r, c + 1, 0) == a + 1, "contiguous within a strip");
                }
        }
        CHECK(hit == elems, "onto: nb=%lld %lld of %lld", (long long)nb, (long long)hit, (long long)elems);
        // a share context stores the tile rows from I0 on: the same map, shifted by bq_sym_off(I0)
        for (int64_t I0 = 0; I0 < nb; I0 += 3)
            for (int64_t I = I0; I < nb; I += 2) {
                const int64_t i = I * T + 17, j = (I + 1) * T - 3;
                CHECK(bq_sym_addr(i, j, I0) == bq_sym_addr(i, j, 0) - bq_sym_off(I0), "origin");
                CHECK(bq_sym_addr(I0 * T, 0, I0) == 0, "first element");
            }
    }
    if (fails) {
        std::printf("sym_layout_check: %d failures\n", fails);
        return 1;
    }
    std::printf("sym_layout_check ok\n");
    return 0;
}
