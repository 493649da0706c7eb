// Host check of the blocked Cholesky's schedule (optiml_amd/csrc/bq_chol_sched.h), the header the kernels decode their block ids
// with and the driver issues its steps from.  Built by tests/test_chol_sched_host.py with ASan + UBSan.
//   decodes   every lower tile is produced by exactly one block id of the launched grid, every other block id by none
//   choices   pinned on both sides of every threshold; the forward sweep's slices are at most four, disjoint, even, and cover the span
//   plan      replayed in issue order for nb = 1 .. 80 block columns, P = 1 .. 4, look-ahead off and on: every tile (i, j) receives
//             the update of every block column k < j exactly once and before the step that consumes it; every image slot read holds
//             the block column the reader expects, for the rows it reads; image offsets and event indices stay in range
//   races     the plan as a partial order (stream order + each wait bound to the latest earlier record of its event): no two
//             unordered steps may touch the same H tile, image slot x row tile or LinvT block unless both only read it
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bq_chol_sched.h"

static int fails = 0;
static bool quiet = false;   // check_the_checker: failures are counted, not printed
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            if (++fails <= 20 && !quiet) {       \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);        \
                std::printf("\n");               \
            }                                    \
        }                                        \
    } while (0)

typedef long long ll;

// ---------------------------------------------------------------------------------------------
static void check_decodes() {
    for (int64_t T = 1; T <= 200; ++T) {
        const int64_t S = (T + 7) / 8;
        for (int order = 0; order < 2; ++order) {
            const int64_t nsuper = order ? bq_chol_nsuper(T, 1) : 0;
            if (order) CHECK(nsuper == S * (S + 1) / 2, "T=%lld", (ll)T);
            const int64_t grid = bq_chol_syrk_grid(T, nsuper);
            CHECK(grid >= T * (T + 1) / 2 && grid < (int64_t)1 << 31, "T=%lld grid=%lld", (ll)T, (ll)grid);
            std::vector<int> hit((size_t)(T * T), 0);
            int64_t none = 0;
            for (int64_t bid = 0; bid < grid; ++bid) {
                int64_t ti = -1, tj = -1;
                if (!bq_chol_syrk_decode(bid, T, nsuper, &ti, &tj)) {
                    ++none;
                    continue;
                }
                if (!(ti >= 0 && ti < T && tj >= 0 && tj <= ti)) {
                    CHECK(false, "syrk order %d T=%lld bid=%lld -> (%lld, %lld)", order, (ll)T, (ll)bid, (ll)ti, (ll)tj);
                    continue;
                }
                ++hit[(size_t)(ti * T + tj)];
            }
            for (int64_t ti = 0; ti < T; ++ti)
                for (int64_t tj = 0; tj <= ti; ++tj)
                    CHECK(hit[(size_t)(ti * T + tj)] == 1, "syrk order %d T=%lld tile (%lld, %lld) x %d", order, (ll)T, (ll)ti, (ll)tj,
                          hit[(size_t)(ti * T + tj)]);
            CHECK(none == grid - T * (T + 1) / 2, "syrk order %d T=%lld", order, (ll)T);
            if (!order) CHECK(none == 0, "row-major grid is exact: T=%lld", (ll)T);
        }
    }
    for (int64_t T = 1; T <= 64; ++T)
        for (int nc = 1; nc <= 8; ++nc) {
            const int64_t grid = bq_chol_head_grid(T, nc);
            int64_t want = 0;
            for (int64_t tj = 0; tj < nc && tj < T; ++tj) want += T - tj;
            CHECK(grid == want, "head grid T=%lld nc=%d", (ll)T, nc);
            std::vector<int> hit((size_t)(T * T), 0);
            for (int64_t b = 0; b < grid; ++b) {
                int64_t ti = -1, tj = -1;
                if (!bq_chol_head_decode(b, T, nc, &ti, &tj)) {
                    CHECK(false, "head T=%lld nc=%d block %lld has no tile", (ll)T, nc, (ll)b);
                    continue;
                }
                if (!(ti >= 0 && ti < T && tj >= 0 && tj <= ti && tj < nc)) {
                    CHECK(false, "head T=%lld nc=%d b=%lld -> (%lld, %lld)", (ll)T, nc, (ll)b, (ll)ti, (ll)tj);
                    continue;
                }
                ++hit[(size_t)(ti * T + tj)];
            }
            for (int64_t ti = 0; ti < T; ++ti)
                for (int64_t tj = 0; tj <= ti; ++tj)
                    CHECK(hit[(size_t)(ti * T + tj)] == (tj < nc ? 1 : 0), "head T=%lld nc=%d tile (%lld, %lld)", (ll)T, nc, (ll)ti, (ll)tj);
        }
}

// ---------------------------------------------------------------------------------------------
static void check_choices() {
    // without hooks every choice is the one the sizes were measured for
    CHECK(bq_chol_super_max(24575, false) == 2 && bq_chol_super_max(24576, false) == 4 && bq_chol_super_max(128, true) == 4, "super_max");
    CHECK(bq_chol_passes(128, 2, 0) == 2 && bq_chol_passes(24448, 2, 0) == 2 && bq_chol_passes(24576, 4, 0) == 3, "P");
    CHECK(bq_chol_passes(65408, 4, 0) == 3 && bq_chol_passes(65536, 4, 0) == 4 && bq_chol_passes(65536, 2, 0) == 2, "P");
    for (int h = 1; h <= 4; ++h) CHECK(bq_chol_passes(1280, 4, h) == h && bq_chol_passes(1280, 2, h) == (h < 2 ? h : 2), "P hook %d", h);
    CHECK(bq_chol_passes(1280, 4, 5) == 2 && bq_chol_passes(1280, 4, -1) == 2, "P hook out of range");
    CHECK(!bq_chol_use_lookahead(15 * 128, true, -1) && bq_chol_use_lookahead(16 * 128, true, -1), "look-ahead by size");
    CHECK(!bq_chol_use_lookahead(1 << 20, false, -1) && !bq_chol_use_lookahead(1 << 20, false, 1), "look-ahead needs the workspace's streams");
    CHECK(!bq_chol_use_lookahead(1 << 20, true, 0) && bq_chol_use_lookahead(128, true, 1), "look-ahead hook");
    CHECK(BQ_CHOL_SUPER_MIN == 4096 && bq_chol_nsuper(90, BQ_CHOL_SUPER_MIN) == 0 && bq_chol_nsuper(91, BQ_CHOL_SUPER_MIN) == 78, "nsuper");
    CHECK(bq_chol_nsuper(21, 1) == 6 && bq_chol_syrk_grid(21, 6) == 512 && bq_chol_syrk_grid(91, 78) == 80 * 64, "super-tile grid");
    CHECK(bq_chol_big_block(4095, 0) == 1024 && bq_chol_big_block(4096, 0) == 2048 && bq_chol_big_block(8191, 0) == 2048 &&
              bq_chol_big_block(8192, 0) == 4096,
          "big block");
    CHECK(bq_chol_big_block(128, 4096) == 4096 && bq_chol_big_block(128, 8192) == 8192 && bq_chol_big_block(128, 512) == 1024, "big block hook");
    int s = 0;
    int64_t w = 0;
    bq_chol_fwd_slices(16384, BQ_CHOL_FWD_SLICE, &s, &w);
    CHECK(s == 1 && w == 16384, "one slice up to 16384 columns");
    bq_chol_fwd_slices(16512, BQ_CHOL_FWD_SLICE, &s, &w);
    CHECK(s == 2 && w == 8704, "two slices: %d x %lld", s, (ll)w);
    bq_chol_fwd_slices(49920, BQ_CHOL_FWD_SLICE, &s, &w);
    CHECK(s == 4 && w == 12800, "four slices: %d x %lld", s, (ll)w);
    for (int64_t unit : {(int64_t)512, (int64_t)16384})
        for (int64_t span = 128; span <= 70000; span += 128)
            for (int64_t kb : {(int64_t)0, (int64_t)640}) {
                const int64_t k0 = kb + span;
                bq_chol_fwd_slices(span, unit, &s, &w);
                CHECK(s >= 1 && s <= BQ_CHOL_MAX_SLICES && w % 512 == 0, "span=%lld unit=%lld: %d x %lld", (ll)span, (ll)unit, s, (ll)w);
                int64_t at = kb;   // the slices, in order, tile [kb, k0): disjoint and complete
                for (int y = 0; y < s; ++y) {
                    int64_t lo = 0, hi = 0;
                    bq_chol_fwd_slice_range(kb, k0, w, y, &lo, &hi);
                    CHECK(lo % 2 == 0, "even start: span=%lld unit=%lld y=%d", (ll)span, (ll)unit, y);
                    if (hi <= lo) continue;   // an empty slice: its workgroups add nothing
                    CHECK(lo == at && hi <= k0, "span=%lld unit=%lld y=%d [%lld, %lld) after %lld", (ll)span, (ll)unit, y, (ll)lo, (ll)hi, (ll)at);
                    at = hi;
                }
                CHECK(at == k0, "cover: span=%lld unit=%lld ends at %lld", (ll)span, (ll)unit, (ll)at);
            }
}

// ---------------------------------------------------------------------------------------------
// one plan: replay in issue order, then the race check
// ---------------------------------------------------------------------------------------------
struct Bits {   // a footprint
    std::vector<uint64_t> w;
    explicit Bits(size_t n) : w((n + 63) / 64, 0) {}
    void set(size_t i) { w[i / 64] |= (uint64_t)1 << (i % 64); }
    bool meets(const Bits &o) const {
        for (size_t i = 0; i < w.size(); ++i)
            if (w[i] & o.w[i]) return true;
        return false;
    }
};

static std::vector<bq_chol_step> plan_of(int64_t nb, int P, bool la) {
    std::vector<bq_chol_step> plan;
    // the super-tile order from 10 tiles on: both orders of the rest update appear in the plans
    bq_chol_plan(nb * BQ_CHOL_NB, P, la, 10, [&](const bq_chol_step &s) { plan.push_back(s); });
    return plan;
}

static void check_plan(const std::vector<bq_chol_step> &plan, int64_t nb, int P, bool la) {
    const int64_t np = nb * BQ_CHOL_NB;
    const int super_max = BQ_CHOL_MAX_PASSES;                 // what a workspace created under the chol_passes hook holds
    const int64_t nslot = 2 * super_max * 2;                   // 128-row image slots
    const size_t ns = plan.size();
#define WHERE "nb=%lld P=%d la=%d step %zu op %d", (ll)nb, P, (int)la, si, s.op

    // footprints: H tiles, then image slot x row tile, then LinvT blocks
    const size_t oH = 0, oI = (size_t)(nb * nb), oL = oI + (size_t)(nslot * nb), nbits = oL + (size_t)nb;
    std::vector<Bits> rd(ns, Bits(nbits)), wr(ns, Bits(nbits));

    std::vector<int> upd((size_t)(nb * nb * nb), 0);          // upd[(i * nb + j) * nb + k]: updates of tile (i, j) by block column k
    std::vector<int> final_((size_t)(nb * nb), 0);             // tile holds its part of the factor
    std::vector<int64_t> slot_col((size_t)(nslot * nb), -1);   // block column whose image slot s holds for row tile r
    std::vector<int> linv((size_t)nb, 0);
    auto current = [&](int64_t i, int64_t j) {   // tile (i, j) has received every update k < j exactly once
        for (int64_t k = 0; k < j; ++k)
            if (upd[(size_t)((i * nb + j) * nb + k)] != 1) return false;
        return true;
    };
    for (size_t si = 0; si < ns; ++si) {
        const bq_chol_step &s = plan[si];
        CHECK(s.stream >= 0 && s.stream <= 2 && (la || s.stream == BQ_CHOL_ON_CTX), WHERE);
        if (s.op == BQ_CHOL_RECORD || s.op == BQ_CHOL_WAIT) {
            CHECK(la && s.nc >= 0 && s.nc < BQ_CHOL_EVENTS, WHERE);
            continue;
        }
        CHECK(s.row % BQ_CHOL_NB == 0 && s.row >= 0 && s.row < np, WHERE);
        const int64_t k = s.row / BQ_CHOL_NB;
        if (s.op == BQ_CHOL_DIAG) {
            CHECK(current(k, k) && !final_[(size_t)(k * nb + k)], WHERE);
            final_[(size_t)(k * nb + k)] = 1;
            linv[(size_t)k] = 1;
            rd[si].set(oH + (size_t)(k * nb + k));
            wr[si].set(oH + (size_t)(k * nb + k));
            wr[si].set(oL + (size_t)k);
            continue;
        }
        CHECK(s.img >= 0 && s.img % BQ_CHOL_NB == 0 && s.kdim >= BQ_CHOL_NB && s.kdim % BQ_CHOL_NB == 0 &&
                  s.img + s.kdim <= 2 * super_max * 256,
              WHERE);
        if (s.img < 0 || s.img + s.kdim > 2 * super_max * 256) continue;
        const int64_t slot0 = s.img / BQ_CHOL_NB, nk = s.kdim / BQ_CHOL_NB;
        if (s.op == BQ_CHOL_TRSM) {
            CHECK(s.T == nb - k - 1 && s.T >= 1 && nk == 1 && linv[(size_t)k] && final_[(size_t)(k * nb + k)], WHERE);
            rd[si].set(oL + (size_t)k);
            for (int64_t r = k + 1; r < nb; ++r) {
                CHECK(current(r, k) && !final_[(size_t)(r * nb + k)], WHERE);
                final_[(size_t)(r * nb + k)] = 1;
                slot_col[(size_t)(slot0 * nb + r)] = k;
                rd[si].set(oH + (size_t)(r * nb + k));
                wr[si].set(oH + (size_t)(r * nb + k));
                wr[si].set(oI + (size_t)(slot0 * nb + r));
            }
            continue;
        }
        // an update of the trailing matrix at tile k: its tiles from the kernel's own decode
        CHECK(s.T == nb - k && s.T >= 1, WHERE);
        int64_t grid = 0;
        if (s.op == BQ_CHOL_COL) {
            CHECK(nk == 1 && s.nc == 1, WHERE);
            grid = s.T;
        } else if (s.op == BQ_CHOL_HEAD) {
            CHECK(s.nc >= 1 && s.nc <= 2 * BQ_CHOL_MAX_PASSES, WHERE);
            grid = bq_chol_head_grid(s.T, (int)s.nc);
        } else if (s.op == BQ_CHOL_REST) {
            CHECK(s.nc == bq_chol_nsuper(s.T, 10), WHERE);
            grid = bq_chol_syrk_grid(s.T, s.nc);
        } else {
            CHECK(false, WHERE);
        }
        for (int64_t b = 0; b < grid; ++b) {
            int64_t ti = 0, tj = 0;
            if (s.op == BQ_CHOL_COL) {
                ti = b;
            } else if (s.op == BQ_CHOL_HEAD) {
                if (!bq_chol_head_decode(b, s.T, (int)s.nc, &ti, &tj)) continue;
            } else if (!bq_chol_syrk_decode(b, s.T, s.nc, &ti, &tj)) {
                continue;
            }
            const int64_t i = k + ti, j = k + tj;
            CHECK(!final_[(size_t)(i * nb + j)], WHERE);
            rd[si].set(oH + (size_t)(i * nb + j));
            wr[si].set(oH + (size_t)(i * nb + j));
            for (int64_t t = 0; t < nk; ++t) {
                // slot t holds, for both operand rows, the same factored block column; the columns of one read are consecutive
                const int64_t ci = slot_col[(size_t)((slot0 + t) * nb + i)], cj = slot_col[(size_t)((slot0 + t) * nb + j)];
                const int64_t c0 = slot_col[(size_t)(slot0 * nb + i)];
                CHECK(ci >= 0 && ci == cj && ci == c0 + t && ci < j, "image: nb=%lld P=%d la=%d step %zu tile (%lld, %lld) slot %lld holds %lld / %lld",
                      (ll)nb, P, (int)la, si, (ll)i, (ll)j, (ll)(slot0 + t), (ll)ci, (ll)cj);
                if (ci < 0 || ci >= nb) continue;
                CHECK(final_[(size_t)(i * nb + ci)] && final_[(size_t)(j * nb + ci)], WHERE);
                ++upd[(size_t)((i * nb + j) * nb + ci)];
                rd[si].set(oI + (size_t)((slot0 + t) * nb + i));
                rd[si].set(oI + (size_t)((slot0 + t) * nb + j));
            }
        }
    }
    for (int64_t i = 0; i < nb; ++i)
        for (int64_t j = 0; j <= i; ++j) {
            CHECK(final_[(size_t)(i * nb + j)] == 1, "nb=%lld P=%d la=%d tile (%lld, %lld) never factored", (ll)nb, P, (int)la, (ll)i, (ll)j);
            for (int64_t k = 0; k < nb; ++k)
                CHECK(upd[(size_t)((i * nb + j) * nb + k)] == (k < j ? 1 : 0), "nb=%lld P=%d la=%d tile (%lld, %lld) column %lld x %d", (ll)nb, P,
                      (int)la, (ll)i, (ll)j, (ll)k, upd[(size_t)((i * nb + j) * nb + k)]);
        }

    // the partial order as vector clocks over the three streams: step a precedes step b iff clock_b[stream_a] >= seq_a
    struct Clock {
        int64_t c[3];
    };
    std::vector<Clock> clk(ns);
    Clock now[3] = {{{0, 0, 0}}, {{0, 0, 0}}, {{0, 0, 0}}};
    Clock recorded[BQ_CHOL_EVENTS];
    bool has_record[BQ_CHOL_EVENTS] = {false, false, false, false, false, false, false, false};
    for (size_t si = 0; si < ns; ++si) {
        const bq_chol_step &s = plan[si];
        if (s.stream < 0 || s.stream > 2) continue;
        Clock &c = now[s.stream];
        if (s.op == BQ_CHOL_WAIT && s.nc >= 0 && s.nc < BQ_CHOL_EVENTS) {
            CHECK(has_record[s.nc], WHERE);   // a wait for an event never recorded orders nothing
            if (has_record[s.nc])
                for (int t = 0; t < 3; ++t)
                    if (recorded[s.nc].c[t] > c.c[t]) c.c[t] = recorded[s.nc].c[t];
        }
        ++c.c[s.stream];
        clk[si] = c;
        if (s.op == BQ_CHOL_RECORD && s.nc >= 0 && s.nc < BQ_CHOL_EVENTS) {
            recorded[s.nc] = c;
            has_record[s.nc] = true;
        }
    }
    auto before = [&](size_t a, size_t b) { return clk[b].c[plan[a].stream] >= clk[a].c[plan[a].stream]; };
    for (size_t a = 0; a < ns; ++a)
        for (size_t b = a + 1; b < ns; ++b) {
            if (before(a, b)) continue;
            const bool clash = wr[a].meets(wr[b]) || wr[a].meets(rd[b]) || rd[a].meets(wr[b]);
            CHECK(!clash, "race: nb=%lld P=%d la=%d steps %zu (op %d row %lld stream %d) and %zu (op %d row %lld stream %d) are unordered", (ll)nb,
                  P, (int)la, a, plan[a].op, (ll)plan[a].row, plan[a].stream, b, plan[b].op, (ll)plan[b].row, plan[b].stream);
        }
    if (la && ns >= 2) {   // what was enqueued before precedes every step, and every step precedes what is enqueued after
        CHECK(plan[0].op == BQ_CHOL_RECORD && plan[0].stream == BQ_CHOL_ON_CTX && plan[ns - 1].op == BQ_CHOL_WAIT &&
                  plan[ns - 1].stream == BQ_CHOL_ON_CTX,
              "nb=%lld P=%d: the context stream opens and closes the plan", (ll)nb, P);
        for (size_t a = 1; a + 1 < ns; ++a) CHECK(before(0, a) && before(a, ns - 1), "nb=%lld P=%d step %zu is not fenced", (ll)nb, P, a);
    }
#undef WHERE
}

// the checks must be able to fail: plans with one defect each are reported
static void check_the_checker() {
    const int before = fails;
    const int64_t nb = 20;
    const std::vector<bq_chol_step> good = plan_of(nb, 2, true);
    int streams = 0;
    for (const bq_chol_step &s : good) streams |= 1 << s.stream;
    CHECK(streams == 7, "a look-ahead plan uses all three streams");
    check_plan(good, nb, 2, true);
    CHECK(fails == before, "the unchanged plan passes");
    auto broken = [&](const char *what, auto &&change) {
        std::vector<bq_chol_step> plan = good;
        change(plan);
        const int f0 = fails;
        quiet = true;
        check_plan(plan, nb, 2, true);
        quiet = false;
        const int found = fails - f0;
        fails = f0;
        CHECK(found > 0, "a plan with %s passes the check", what);
    };
    auto find = [&](const std::vector<bq_chol_step> &plan, int op, int stream, int nth) {
        for (size_t i = 0; i < plan.size(); ++i)
            if (plan[i].op == op && plan[i].stream == stream && nth-- == 0) return i;
        return plan.size();
    };
    broken("a side stream that does not wait for the head update", [&](std::vector<bq_chol_step> &p) {
        p.erase(p.begin() + (long)find(p, BQ_CHOL_WAIT, BQ_CHOL_ON_SIDE, 1));
    });
    broken("a main stream that does not wait for the narrow chain", [&](std::vector<bq_chol_step> &p) {
        p.erase(p.begin() + (long)find(p, BQ_CHOL_WAIT, BQ_CHOL_ON_MAIN, 2));
    });
    broken("a rest update issued twice", [&](std::vector<bq_chol_step> &p) {
        const size_t i = find(p, BQ_CHOL_REST, BQ_CHOL_ON_MAIN, 0);
        p.insert(p.begin() + (long)i, p[i]);
    });
    broken("a head update left out", [&](std::vector<bq_chol_step> &p) { p.erase(p.begin() + (long)find(p, BQ_CHOL_HEAD, BQ_CHOL_ON_MAIN, 1)); });
    broken("an image written into the other buffer", [&](std::vector<bq_chol_step> &p) { p[find(p, BQ_CHOL_TRSM, BQ_CHOL_ON_SIDE, 0)].img += 512; });
}

int main() {
    check_decodes();
    check_choices();
    check_the_checker();
    for (int64_t nb = 1; nb <= 80; ++nb)
        for (int P = 1; P <= BQ_CHOL_MAX_PASSES; ++P)
            for (int la = 0; la < 2; ++la) check_plan(plan_of(nb, P, la != 0), nb, P, la != 0);
    if (fails) {
        std::printf("chol_sched_check: %d failures\n", fails);
        return 1;
    }
    std::printf("chol_sched_check ok\n");
    return 0;
}
