// bq_mrsmo_resolve (optiml_amd/csrc/bq_mrsmo_cache.h) on the host for tests/test_mrsmo_cache_host.py: reads "n R calls", then per
// call "np pin_row .. m row .." (-1: none); prints per call the slots | the miss list row:slot | the running hits and misses.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bq_mrsmo_cache.h"

static long long next_int() {
    long long v = 0;
    if (std::scanf("%lld", &v) != 1) {
        std::fprintf(stderr, "short input\n");
        std::exit(2);
    }
    return v;
}

int main() {
    const long long n = next_int(), R = next_int(), calls = next_int();
    std::vector<int> slot_of((size_t)n, -1), row_of((size_t)R, -1);
    std::vector<long long> stamp((size_t)R, 0);
    bq_mrsmo_cache c = {R, 0, 0, 0, 0, slot_of.data(), row_of.data(), stamp.data()};
    bq_mrsmo_serial par;
    for (long long q = 0; q < calls; ++q) {
        const int np = (int)next_int();
        std::vector<int> pin((size_t)np);
        for (int &p : pin) {
            const long long row = next_int();
            p = row < 0 ? -1 : slot_of[(size_t)row];
        }
        const int m = (int)next_int();
        std::vector<int> req((size_t)m), slot((size_t)m, -2), miss_row((size_t)m), miss_slot((size_t)m);
        for (int &r : req) r = (int)next_int();
        int n_miss = -1;
        bq_mrsmo_resolve(&c, np, pin.data(), m, req.data(), slot.data(), miss_row.data(), miss_slot.data(), &n_miss, par);
        for (int u = 0; u < m; ++u) std::printf(u + 1 < m ? "%d " : "%d |", slot[(size_t)u]);
        for (int u = 0; u < n_miss; ++u) std::printf(" %d:%d", miss_row[(size_t)u], miss_slot[(size_t)u]);
        std::printf(" | %lld %lld\n", c.hits, c.misses);
    }
    std::printf("mrsmo_cache_check ok\n");
    return 0;
}
