// A dense host solver around optiml_amd/csrc/bq_rsmo_step.h — the scalar rules the device solver (bq_rsmo.hip) runs — held by
// tests/test_rsmo_step_host.py to the NumPy restatement (tests/smo_rows_reference.py): the same pair sequence, alpha and G bit for
// bit.  Scans run in ascending t through the header's combines; built with -ffp-contract=off (no product is fused with a sum).
//   rsmo_step_check solve  < "n N tol cap" K (n x n) signs (N) p (N) C (N), numbers as hex floats
//   rsmo_step_check victim < "R m" then m requests "row keep_row" (keep_row -1: none): the cache of bq_rsmo.hip under the victim rule
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "bq_rsmo_step.h"

static double next_double() {
    std::string tok;
    if (!(std::cin >> tok)) {
        std::fprintf(stderr, "short input\n");
        std::exit(2);
    }
    return std::strtod(tok.c_str(), nullptr);
}

static void print_hex(const std::vector<double> &v) {
    for (size_t q = 0; q < v.size(); ++q) std::printf("%s%a", q ? " " : "", v[q]);
    std::printf("\n");
}

static int solve() {
    const long long n = (long long)next_double(), N = (long long)next_double();
    const double tol = next_double();
    const long long cap = (long long)next_double();
    if (n < 2 || (N != n && N != 2 * n)) return 2;
    std::vector<double> K((size_t)(n * n)), y((size_t)N), p((size_t)N), C((size_t)N);
    for (auto &v : K) v = next_double();
    for (auto &v : y) v = next_double();
    for (auto &v : p) v = next_double();
    for (auto &v : C) v = next_double();
    std::vector<double> alpha((size_t)N, 0.0), G(p), QD((size_t)n);
    for (long long t = 0; t < n; ++t) QD[t] = K[t * n + t];
    std::vector<long long> pairs;
    long long steps = 0;
    int status = 0;
    double gmax = -BQ_RSMO_INF, gmax2 = -BQ_RSMO_INF;
    for (;;) {
        bq_rsmo_pick up = {-BQ_RSMO_INF, -1};
        double low = -BQ_RSMO_INF;
        for (long long v = 0; v < N; ++v) {
            if (bq_rsmo_in_up(y[v], alpha[v], C[v])) {
                const double val = bq_rsmo_up_value(y[v], G[v]);
                if (bq_rsmo_max_before(val, v, up.v, up.idx)) up = {val, v};
            }
            if (bq_rsmo_in_low(y[v], alpha[v], C[v])) {
                const double val = bq_rsmo_low_value(y[v], G[v]);
                low = val > low ? val : low;
            }
        }
        gmax = up.v;
        gmax2 = low;
        if (up.idx < 0 || bq_rsmo_stop(gmax, gmax2, tol)) {
            status = 1;
            break;
        }
        if (steps >= cap) {
            status = 2;
            break;
        }
        const long long i = up.idx, r = i % n;
        bq_rsmo_pick best = {BQ_RSMO_INF, -1};
        for (long long v = 0; v < N; ++v) {
            if (!bq_rsmo_in_low(y[v], alpha[v], C[v])) continue;
            bool ok;
            const double sc = bq_rsmo_score(gmax, y[v], G[v], QD[r], QD[v % n], K[r * n + v % n], &ok);
            if (ok && bq_rsmo_min_before(sc, v, best.v, best.idx)) best = {sc, v};
        }
        if (best.idx < 0) {
            status = 1;
            break;
        }
        const long long j = best.idx, rj = j % n;
        const double old_i = alpha[i], old_j = alpha[j];
        bq_rsmo_pair_update(y[i], y[j], G[i], G[j], QD[r], QD[rj], K[r * n + rj], C[i], C[j], &alpha[i], &alpha[j]);
        const double d_i = alpha[i] - old_i, d_j = alpha[j] - old_j;
        for (long long v = 0; v < N; ++v) {
            const double s_i = y[i] * y[v], s_j = y[j] * y[v];
            const double q_i = s_i * K[r * n + v % n], q_j = s_j * K[rj * n + v % n];
            G[v] = bq_rsmo_grad(G[v], q_i, d_i, q_j, d_j);
        }
        pairs.push_back(i);
        pairs.push_back(j);
        steps += 1;
    }
    bq_rsmo_rho rho;
    for (long long v = 0; v < N; ++v) bq_rsmo_rho_add(&rho, y[v], alpha[v], C[v], G[v]);
    std::printf("%lld %d\n", steps, status);
    for (size_t q = 0; q < pairs.size(); ++q) std::printf("%s%lld", q ? " " : "", pairs[q]);
    std::printf("\n");
    print_hex(alpha);
    print_hex(G);
    std::printf("%a %a %a\n", bq_rsmo_rho_value(&rho), gmax, gmax2);
    return 0;
}

// the tables of the device cache (slot_of, row_of, stamp, the clock and the count of slots ever used), one request at a time
static int victim() {
    const long long R = (long long)next_double(), m = (long long)next_double();
    if (R < 2) return 2;
    std::vector<long long> stamp((size_t)R, 0), row_of((size_t)R, -1);
    long long clock = 0;
    for (long long q = 0; q < m; ++q) {
        const long long row = (long long)next_double(), keep_row = (long long)next_double();
        long long have = -1, keep = -1;
        for (long long s = 0; s < R; ++s) {
            if (row_of[s] == row) have = s;
            if (keep_row >= 0 && row_of[s] == keep_row) keep = s;
        }
        long long slot = have;
        if (have < 0) {
            slot = bq_rsmo_victim(stamp.data(), R, keep);
            if (slot < 0 || slot == keep) return 3;
            row_of[slot] = row;
        }
        stamp[slot] = ++clock;
        std::printf("%lld %d\n", slot, have >= 0 ? 1 : 0);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const int rc = std::strcmp(argv[1], "solve") == 0 ? solve() : std::strcmp(argv[1], "victim") == 0 ? victim() : 2;
    if (rc == 0) std::printf("rsmo_step_check ok\n");
    return rc;
}
