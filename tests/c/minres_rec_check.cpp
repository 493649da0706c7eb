// A dense host MINRES around optiml_amd/csrc/bq_minres_rec.h (the scalar recurrence the three device forms share), for
// tests/test_minres_rec_host.py: reads  n  maxiter  rtol  A (n x n, row-major)  b (n)  as text (strtod: hex floats are exact),
// runs scipy's iteration (x0 = 0, no shift, no preconditioner) and prints  itn  istop  x.  The vector part is written out here as
// scipy has it; everything scalar is the header's.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bq_minres_rec.h"

static double dot(const std::vector<double> &a, const std::vector<double> &b) {
    double s = 0.0;
    for (size_t i = 0; i < a.size(); ++i) s += a[i] * b[i];
    return s;
}

int main() {
    int n = 0;
    long long maxiter = 0;
    double rtol = 0.0;
    if (scanf("%d %lld", &n, &maxiter) != 2 || n < 1 || n > 4096) return 2;
    auto number = [](double *out) {
        char tok[64];
        if (scanf("%63s", tok) != 1) return false;
        char *end = nullptr;
        *out = strtod(tok, &end);
        return end != tok && *end == '\0';
    };
    if (!number(&rtol)) return 2;
    std::vector<double> A((size_t)n * n), b(n);
    for (double &a : A)
        if (!number(&a)) return 2;
    for (double &v : b)
        if (!number(&v)) return 2;

    std::vector<double> x(n, 0.0), r1 = b, r2 = b, y = b, v(n), w(n, 0.0), w1(n, 0.0), w2(n, 0.0);
    bq_minres_rec m;
    m.start(dot(r1, y));
    long long itn = 0;
    if (m.beta1 > 0.0) {
        while (itn < maxiter) {
            itn += 1;
            const double s = 1.0 / m.beta;
            for (int i = 0; i < n; ++i) v[i] = s * y[i];
            for (int i = 0; i < n; ++i) {
                double acc = 0.0;
                for (int j = 0; j < n; ++j) acc += A[(size_t)i * n + j] * v[j];
                y[i] = acc;
            }
            if (itn >= 2) {
                const double c = m.beta / m.oldb;
                for (int i = 0; i < n; ++i) y[i] -= c * r1[i];
            }
            const double alfa = dot(v, y);
            const double c = alfa / m.beta;
            for (int i = 0; i < n; ++i) y[i] -= c * r2[i];
            r1 = r2;
            r2 = y;
            const double beta2 = dot(r2, y);
            if (beta2 < 0.0) {
                m.istop = 7;
                break;
            }
            m.rotate(alfa, beta2, itn);
            w1 = w2;
            w2 = w;
            for (int i = 0; i < n; ++i) {
                w[i] = (v[i] - m.oldeps * w1[i] - m.delta * w2[i]) * m.denom;
                x[i] += m.phi * w[i];
            }
            if (m.stop(dot(x, x), itn, maxiter, rtol) != 0) break;
        }
    }
    printf("%lld %d", itn, m.istop);
    for (int i = 0; i < n; ++i) printf(" %a", x[i]);
    printf("\nminres_rec_check ok\n");
    return 0;
}
