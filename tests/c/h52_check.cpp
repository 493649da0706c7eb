// Host check of the Hessian image format (optiml_amd/csrc/bq_h52.h): the 52-bit code of h = fl(K + 1), its escape for h = 2.0, the
// refusals of encode, the lane order of a tile row and, composed with the offsets of bq_sym_addr, that every element's three plane
// accesses stay inside the 6.5-byte allocation.  Built by tests/test_h52_host.py with ASan + UBSan and run on its own.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "bq_h52.h"

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

static uint64_t bits_of(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}
static double value_of(uint64_t b) {
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

// encode -> the three plane fields -> decode
static bool round_trip(double h, uint64_t *code_out = nullptr) {
    bool bad = false;
    const uint64_t code = bq_h52_encode(bits_of(h), &bad);
    if (code_out) *code_out = code;
    if (bad || (code >> 52) != 0) return false;
    const uint64_t back = bq_h52_bits((uint32_t)code, (uint32_t)(code >> 32) & 0xFFFFu, (uint32_t)(code >> 48) & 0xFu);
    return back == bits_of(h);
}
static bool refused(double h) {
    bool bad = false;
    const uint64_t code = bq_h52_encode(bits_of(h), &bad);
    return bad && code == 0;
}

int main() {
    // the named values
    const double named[] = {1.0, 2.0, 1.0 + 0x1p-15, 1.0 + 0x1p-14, 2.0 - 0x1p-52, (1.0 - 0x1p-53) + 1.0, 0.5 + 1.0, 0x1p-14 + 1.0};
    for (double h : named) CHECK(round_trip(h), "h=%a", h);
    CHECK((1.0 - 0x1p-53) + 1.0 == 2.0, "fl(k + 1) of the largest k < 1 is 2.0");
    uint64_t code = 99;
    CHECK(round_trip(1.0, &code) && code == 0, "1.0 is the zero code (the panel's zero pad, a memset image)");
    CHECK(round_trip(2.0, &code) && code == 1, "2.0 takes the escape code");
    CHECK(bq_h52_bits(0, 0, 0) == BQ_H52_ONE && bq_h52_bits(1, 0, 0) == BQ_H52_TWO, "decode of the two special codes");
    // a few million random K in [2^-15, 1]: log-uniform, uniform, and the neighbourhood of both ends (xorshift64*: no library state)
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 0x2545F4914F6CDD1Dull;
    };
    auto unit = [&]() { return (double)(next() >> 11) * 0x1p-53; };   // [0, 1)
    int64_t escapes = 0;
    for (int64_t i = 0; i < 4000000; ++i) {
        double k;
        switch (i & 3) {
            case 0: k = std::exp2(-15.0 * unit()); break;
            case 1: k = 0x1p-15 + (1.0 - 0x1p-15) * unit(); break;
            case 2: k = 1.0 - unit() * 0x1p-40; break;
            default: k = 0x1p-15 * (1.0 + unit() * 0x1p-20); break;
        }
        if (k < 0x1p-15) k = 0x1p-15;
        if (k > 1.0) k = 1.0;
        const double h = k + 1.0;
        CHECK(round_trip(h, &code), "k=%a h=%a", k, h);
        CHECK((code == 1) == (h == 2.0), "the code 1 is produced only by 2.0: k=%a code=%llx", k, (unsigned long long)code);
        escapes += code == 1;
    }
    CHECK(escapes > 0, "the random values reach the escape");
    // every mantissa with one bit set, and its neighbours, from 2^-15 up
    for (int e = 37; e < 52; ++e)
        for (int64_t dlt = -1; dlt <= 1; ++dlt) {
            const uint64_t m = (1ull << e) + (uint64_t)dlt;
            if (m < BQ_H52_MIN_MANT) continue;
            CHECK(round_trip(value_of(BQ_H52_ONE | m), &code) && code == m, "mantissa %llx", (unsigned long long)m);
        }
    // outside the domain
    const double out[] = {1.0 + 0x1p-52, 1.0 + 0x1p-16, 1.0 + 0x1p-15 - 0x1p-52, 2.0 + 0x1p-51, 3.0, 4.0, 0.999, 1.0 - 0x1p-53, 0.0, -1.5, -0.0,
                          std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN(),
                          -std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::denorm_min()};
    for (double h : out) CHECK(refused(h), "h=%a must be refused", h);
    CHECK(refused(value_of(BQ_H52_ONE | 1)), "the bit pattern of the escape code itself is refused");

    // lane order: a bijection of the 256 positions of a tile row; position 4 l + {0, 1, 2, 3} = columns 2 l, 2 l + 1, 128 + 2 l, 128 + 2 l + 1
    {
        bool seen[256] = {false};
        for (int c = 0; c < 256; ++c) {
            const int q = bq_h52_pos(c);
            CHECK(q >= 0 && q < 256 && !seen[q], "c=%d q=%d", c, q);
            if (q >= 0 && q < 256) seen[q] = true;
            CHECK(bq_h52_col(q) == c, "inverse c=%d", c);
        }
        for (int l = 0; l < 64; ++l)
            CHECK(bq_h52_col(4 * l) == 2 * l && bq_h52_col(4 * l + 1) == 2 * l + 1 && bq_h52_col(4 * l + 2) == 128 + 2 * l &&
                      bq_h52_col(4 * l + 3) == 129 + 2 * l,
                  "the four columns of lane %d", l);
    }
    // composed with bq_sym_addr at the seam sizes: a bijection onto [0, elems), a tile row's 256 elements stay in one aligned run,
    // and writing / reading every element through the plane views stays inside 6.5 x elems bytes (the sanitizer watches the vector)
    const int64_t T = BQ_SYM_TILE;
    for (int64_t nb : {1, 8, 9, 17})
        for (int64_t I0 : {(int64_t)0, nb / 2}) {
            const int64_t elems = bq_sym_off(nb) - bq_sym_off(I0);
            CHECK(elems % 65536 == 0 && bq_h52_bytes(elems) * 2 == 13 * elems, "nb=%lld", (long long)nb);
            std::vector<unsigned char> img((size_t)bq_h52_bytes(elems), 0);
            std::vector<unsigned char> seen((size_t)elems, 0);
            const int64_t step = nb > 9 ? 5 : 1;   // rows sampled inside a tile at the largest size (every column always)
            for (int64_t I = I0; I < nb; ++I)
                for (int64_t r = 0; r < T; r += (r < 2 || r >= T - 3) ? 1 : step)
                    for (int64_t c = 0; c < bq_sym_cols(I); ++c) {
                        const int64_t a = bq_sym_addr(I * T + r, c, I0), pos = bq_h52_addr(a);
                        if (pos < 0 || pos >= elems) {
                            CHECK(false, "out of range nb=%lld I=%lld r=%lld c=%lld pos=%lld", (long long)nb, (long long)I, (long long)r,
                                  (long long)c, (long long)pos);
                            continue;
                        }
                        CHECK((pos / T) == (a / T), "stays in its tile row's run");
                        CHECK(!seen[(size_t)pos], "twice: nb=%lld pos=%lld", (long long)nb, (long long)pos);
                        seen[(size_t)pos] = 1;
                        // a value that names its element: mantissa from (a + 1), inside the domain
                        const uint64_t m = BQ_H52_MIN_MANT + (uint64_t)(a + 1) * 0x10000FFFull;
                        bq_h52_put(img.data(), elems, pos, m);
                    }
            for (int64_t I = I0; I < nb; ++I)
                for (int64_t r = 0; r < T; r += (r < 2 || r >= T - 3) ? 1 : step)
                    for (int64_t c = 0; c < bq_sym_cols(I); ++c) {
                        const int64_t a = bq_sym_addr(I * T + r, c, I0);
                        const uint64_t m = BQ_H52_MIN_MANT + (uint64_t)(a + 1) * 0x10000FFFull;
                        CHECK(bq_h52_get(img.data(), elems, bq_h52_addr(a)) == (BQ_H52_ONE | m), "read back nb=%lld a=%lld", (long long)nb,
                              (long long)a);
                    }
            // the last element's accesses as the tile product makes them: 16 + 8 + 2 bytes of lane 63 end at the planes' ends
            const bq_h52p v = bq_h52_view(img.data(), elems) + (elems - T);
            CHECK((const unsigned char *)(v.lo + 4 * 63 + 4) == img.data() + 4 * elems, "lo plane end");
            CHECK((const unsigned char *)(v.mid + 4 * 63 + 4) == img.data() + 6 * elems, "mid plane end");
            CHECK(v.nib + 2 * 63 + 2 == img.data() + bq_h52_bytes(elems), "nib plane end");
        }
    if (fails) {
        std::printf("h52_check: %d failures\n", fails);
        return 1;
    }
    std::printf("h52_check ok\n");
    return 0;
}
