// A dense host solver around the general entry's scalar rules in optiml_amd/csrc/bq_rsmo_step.h — libsvm's Solver from a given start
// (alpha0, G0) and Solver_NU — held by tests/test_rsmo_nu_step_host.py to the NumPy restatement (tests/smo_nu_reference.py): the same
// pair sequence, alpha, G, rho and r bit for bit.  Scans run in ascending t through the header's combines; built with
// -ffp-contract=off (no product is fused with a sum).
//   rsmo_nu_step_check solve   < "n N rule tol cap" K (n x n) signs (N) p (N) C (N) alpha0 (N) G0 (N), numbers as hex floats; rule 0
//                                plain, 1 nu
//   rsmo_nu_step_check victim2 < "R m" then m requests "row keep_row_a keep_row_b" (-1: none): the cache under the two-keep victim rule
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
    const int rule = (int)next_double();
    const double tol = next_double();
    const long long cap = (long long)next_double();
    if (n < 2 || (N != n && N != 2 * n) || (rule != 0 && rule != 1)) return 2;
    std::vector<double> K((size_t)(n * n)), y((size_t)N), p((size_t)N), C((size_t)N), alpha((size_t)N), G((size_t)N), QD((size_t)n);
    for (auto &v : K) v = next_double();
    for (auto &v : y) v = next_double();
    for (auto &v : p) v = next_double();
    for (auto &v : C) v = next_double();
    for (auto &v : alpha) v = next_double();
    for (auto &v : G) v = next_double();
    for (long long t = 0; t < n; ++t) QD[t] = K[t * n + t];
    std::vector<long long> pairs;
    long long steps = 0;
    int status = 0;
    // plain: up[0] / low[0] over all variables; nu: [0] the positive sign, [1] the negative
    bq_rsmo_pick up[2];
    double low[2];
    for (;;) {
        up[0] = up[1] = {-BQ_RSMO_INF, -1};
        low[0] = low[1] = -BQ_RSMO_INF;
        for (long long v = 0; v < N; ++v) {
            const int s = rule == 1 && y[v] < 0.0 ? 1 : 0;
            if (bq_rsmo_in_up(y[v], alpha[v], C[v])) {
                const double val = bq_rsmo_up_value(y[v], G[v]);
                if (bq_rsmo_max_before(val, v, up[s].v, up[s].idx)) up[s] = {val, v};
            }
            if (bq_rsmo_in_low(y[v], alpha[v], C[v])) {
                const double val = bq_rsmo_low_value(y[v], G[v]);
                low[s] = val > low[s] ? val : low[s];
            }
        }
        const bool none = up[0].idx < 0 && up[1].idx < 0;
        const bool stop = rule == 1 ? bq_rsmo_nu_stop(up[0].v, low[0], up[1].v, low[1], tol) : bq_rsmo_stop(up[0].v, low[0], tol);
        if (none || stop) {
            status = 1;
            break;
        }
        if (steps >= cap) {
            status = 2;
            break;
        }
        const long long ip = up[0].idx, in = up[1].idx, rp = ip < 0 ? 0 : ip % n, rn = in < 0 ? 0 : in % n;
        const double qd_p = ip < 0 ? 0.0 : QD[rp], qd_n = in < 0 ? 0.0 : QD[rn];
        bq_rsmo_pick best = {BQ_RSMO_INF, -1};
        for (long long v = 0; v < N; ++v) {
            if (!bq_rsmo_in_low(y[v], alpha[v], C[v])) continue;
            bool ok;
            const double k_p = ip < 0 ? 0.0 : K[rp * n + v % n], k_n = in < 0 ? 0.0 : K[rn * n + v % n];
            const double sc = rule == 1 ? bq_rsmo_nu_score(y[v], G[v], up[0].v, qd_p, k_p, up[1].v, qd_n, k_n, QD[v % n], &ok)
                                        : bq_rsmo_score(up[0].v, y[v], G[v], qd_p, QD[v % n], k_p, &ok);
            if (ok && bq_rsmo_min_before(sc, v, best.v, best.idx)) best = {sc, v};
        }
        if (best.idx < 0) {
            status = 1;
            break;
        }
        const long long j = best.idx, rj = j % n;
        const long long i = rule == 1 && y[j] < 0.0 ? in : ip, r = i % n;
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
    std::printf("%lld %d\n", steps, status);
    for (size_t q = 0; q < pairs.size(); ++q) std::printf("%s%lld", q ? " " : "", pairs[q]);
    std::printf("\n");
    print_hex(alpha);
    print_hex(G);
    if (rule == 1) {
        bq_rsmo_nu_rho nu;
        for (long long v = 0; v < N; ++v) bq_rsmo_nu_rho_add(&nu, y[v], alpha[v], C[v], G[v]);
        double rho = 0.0, r = 0.0;
        bq_rsmo_nu_rho_value(&nu, &rho, &r);
        std::printf("%a %a %a %a\n", rho, r, bq_rsmo_nu_gap(up[0].v, low[0]), bq_rsmo_nu_gap(up[1].v, low[1]));
    } else {
        bq_rsmo_rho rho;
        for (long long v = 0; v < N; ++v) bq_rsmo_rho_add(&rho, y[v], alpha[v], C[v], G[v]);
        std::printf("%a %a %a\n", bq_rsmo_rho_value(&rho), up[0].v, low[0]);
    }
    return 0;
}

// the tables of the device cache (row_of, stamp, the clock), one request at a time, with up to two rows whose slots must stay
static int victim2() {
    const long long R = (long long)next_double(), m = (long long)next_double();
    if (R < 3) return 2;
    std::vector<long long> stamp((size_t)R, 0), row_of((size_t)R, -1);
    long long clock = 0;
    for (long long q = 0; q < m; ++q) {
        const long long row = (long long)next_double(), keep_a = (long long)next_double(), keep_b = (long long)next_double();
        long long have = -1, ka = -1, kb = -1;
        for (long long s = 0; s < R; ++s) {
            if (row_of[s] == row) have = s;
            if (keep_a >= 0 && row_of[s] == keep_a) ka = s;
            if (keep_b >= 0 && row_of[s] == keep_b) kb = s;
        }
        long long slot = have;
        if (have < 0) {
            slot = bq_rsmo_victim2(stamp.data(), R, ka, kb);
            if (slot < 0 || slot == ka || slot == kb) return 3;
            row_of[slot] = row;
        }
        stamp[slot] = ++clock;
        std::printf("%lld %d\n", slot, have >= 0 ? 1 : 0);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const int rc = std::strcmp(argv[1], "solve") == 0 ? solve() : std::strcmp(argv[1], "victim2") == 0 ? victim2() : 2;
    if (rc == 0) std::printf("rsmo_nu_step_check ok\n");
    return rc;
}
