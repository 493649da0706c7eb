// Pairwise coupling of one-vs-one Platt probabilities into class probabilities: libsvm's multiclass_probability (svm.cpp; Wu, Lin &
// Weng 2004, second method), what sklearn.svm.SVC(probability=True).predict_proba evaluates per test point.
//
// One wavefront per test point (one 64-thread workgroup), k <= 64 classes, P = k (k - 1) / 2 pair columns in ovo_pairs order; column
// q = (a, b), a < b, has class b positive.  The wave
//   1. maps its P decision values through the pair sigmoids: z = f A + B, s = exp(-z) / (1 + exp(-z)) (z >= 0) or 1 / (1 + exp(z)),
//      clipped to [1e-7, 1 - 1e-7], r[b][a] = s, r[a][b] = 1 - s, into the point's k x k matrix in LDS (row pitch k | 1: a lane
//      walking its row and the wave reading one row both touch every bank once);
//   2. turns r into Q in place: lane t sums Q[t][t] = sum_{j != t} r[j][t]^2 over ascending j and, for j > t, writes
//      Q[t][j] = Q[j][t] = -r[j][t] r[t][j] (the pair {t, j} is lane t's alone, and the products commute, so both entries hold the
//      bits libsvm's two branches give);
//   3. runs libsvm's Gauss-Seidel sweeps, statement for statement: lane t owns p[t], Qp[t] and Q[t][t]; a sweep's Qp[t] is lane
//      t's sequential walk over its row with p[j] read from LDS (one address for the wave: a broadcast), pQp and the largest error
//      are the same sequential walk over 64 LDS values taken by every lane alike, so every lane holds the same bits and the stop
//      test is wave-uniform; step t of a sweep fetches lane t's Qp and Q[t][t] with a lane read and updates every lane's Qp[j], p[j]
//      from row t of Q.
// No fused multiply-adds (the pragma below: the build contracts by default), no tree sums, IEEE division: a NumPy restatement gives
// the same bits and the same sweep count from the same clipped s (R).  No atomics and nothing of another point: a point's result
// has the same bits alone, at any position and in any batch.  The wave leaves when its own point has converged.
#include "bq_common.h"
#include "bq_scratch.h"

#include <algorithm>
#include <cmath>

constexpr int COUPLE_KMAX = 64;
constexpr double COUPLE_CLIP = 1e-7;

// F: the decision value of (point i, column q) at F[i * f_row + q * f_col]; prob: t x k; iters: t or null; R: t x P or null
__global__ __launch_bounds__(64) void couple_kernel(int k, const double *__restrict__ F, long long f_row, long long f_col,
                                                    const double *__restrict__ A, const double *__restrict__ B,
                                                    double *__restrict__ prob, int *__restrict__ iters, double *__restrict__ R) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    const int ld = k | 1, P = k * (k - 1) / 2, lane = threadIdx.x;
    double *M = lds;               // k x ld: r, then Q
    double *vec = lds + k * ld;    // 64: a value per lane for the sequential walks
    const long long pt = blockIdx.x;
    const bool act = lane < k;

    for (int q = lane; q < P; q += 64) {
        int a = 0, rem = q;   // q = (a, b) in ovo_pairs order: row a holds k - 1 - a pairs
        while (rem >= k - 1 - a) {
            rem -= k - 1 - a;
            ++a;
        }
        const int b = a + 1 + rem;
        const double z = F[pt * f_row + q * f_col] * A[q] + B[q];
        double s = z >= 0.0 ? exp(-z) / (1.0 + exp(-z)) : 1.0 / (1.0 + exp(z));
        s = fmin(fmax(s, COUPLE_CLIP), 1.0 - COUPLE_CLIP);
        if (R) R[pt * P + q] = s;
        M[b * ld + a] = s;
        M[a * ld + b] = 1.0 - s;
    }
    __syncthreads();
    double qtt = 0.0;
    if (act) {
        for (int j = 0; j < k; ++j)
            if (j != lane) qtt += M[j * ld + lane] * M[j * ld + lane];
    }
    __syncthreads();   // every lane has read its column of r: the rows may turn into Q
    if (act) {
        for (int j = lane + 1; j < k; ++j) {
            const double v = -M[j * ld + lane] * M[lane * ld + j];
            M[lane * ld + j] = v;
            M[j * ld + lane] = v;
        }
        M[lane * ld + lane] = qtt;
    }
    __syncthreads();

    double p = 1.0 / k, Qp = 0.0;
    const double eps = 0.005 / k;
    const int max_iter = k > 100 ? k : 100;
    int iter = 0;
    for (; iter < max_iter; ++iter) {
        vec[lane] = act ? p : 0.0;
        __syncthreads();
        Qp = 0.0;
        if (act) {
            for (int j = 0; j < k; ++j) Qp += M[lane * ld + j] * vec[j];
        }
        __syncthreads();
        vec[lane] = act ? p * Qp : 0.0;
        __syncthreads();
        double pQp = 0.0;
        for (int t = 0; t < k; ++t) pQp += vec[t];
        __syncthreads();
        vec[lane] = act ? fabs(Qp - pQp) : 0.0;
        __syncthreads();
        double max_error = 0.0;
        for (int t = 0; t < k; ++t) {
            const double error = vec[t];
            if (error > max_error) max_error = error;
        }
        __syncthreads();
        if (max_error < eps) break;   // the same bits in every lane
        for (int t = 0; t < k; ++t) {
            const double Qpt = __shfl(Qp, t, 64), Qtt = __shfl(qtt, t, 64);
            const double diff = (-Qpt + pQp) / Qtt;
            if (lane == t) p += diff;
            pQp = (pQp + diff * (diff * Qtt + 2.0 * Qpt)) / (1.0 + diff) / (1.0 + diff);
            if (act) {
                Qp = (Qp + diff * M[t * ld + lane]) / (1.0 + diff);
                p /= (1.0 + diff);
            }
        }
    }
    if (act) prob[pt * k + lane] = p;
    if (iters && lane == 0) iters[pt] = iter;
}

static int couple_check(const bq_ctx *c, int ncls, int64_t t, const void *F, const double *A, const double *B, const double *prob) {
    BQ_ARG(c && F && A && B && prob, "NULL argument");
    BQ_ARG(ncls >= 2, "ncls must be >= 2");
    BQ_ARG(ncls <= COUPLE_KMAX, "pairwise coupling takes at most 64 classes");
    BQ_ARG(t >= 1, "t must be >= 1");
    return BQ_OK;
}

static int couple_launch(int k, int64_t points, const double *F, int64_t f_row, int64_t f_col, const double *A, const double *B,
                         double *prob, int *iters, double *R, hipStream_t st) {
    const size_t lds = sizeof(double) * ((size_t)k * (size_t)(k | 1) + 64);
    couple_kernel<<<(unsigned)points, 64, lds, st>>>(k, F, (long long)f_row, (long long)f_col, A, B, prob, iters, R);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

// the device side of both entries: the sigmoids, and the three outputs on the device until the caller's rows are done
struct couple_buffers {
    int k = 0;
    int64_t t = 0, P = 0;
    bq_scratch mem;   // every device buffer of the call, the caller's own included: freed when the buffers go out of scope
    double *A = nullptr, *B = nullptr, *prob = nullptr, *R = nullptr;
    int *iters = nullptr;

    int alloc(int ncls, int64_t points, const double *hA, const double *hB, bool want_R, hipStream_t st) {
        k = ncls;
        t = points;
        P = (int64_t)ncls * (ncls - 1) / 2;
        A = mem.dev<double>(P);
        B = mem.dev<double>(P);
        prob = mem.dev<double>(t * k);
        iters = mem.dev<int>(t);
        if (want_R) R = mem.dev<double>(t * P);
        hipError_t e = mem.error();
        if (e == hipSuccess) e = hipMemcpyAsync(A, hA, sizeof(double) * P, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(B, hB, sizeof(double) * P, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) {
            bq_set_error("pairwise coupling setup failed: %s", hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
        }
        return BQ_OK;
    }
    int download(double *hprob, int *hiters, double *hR, hipStream_t st) {
        hipError_t e = hipMemcpyAsync(hprob, prob, sizeof(double) * t * k, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && hiters) e = hipMemcpyAsync(hiters, iters, sizeof(int) * t, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && hR) e = hipMemcpyAsync(hR, R, sizeof(double) * t * P, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) {
            bq_set_error("pairwise coupling: %s", hipGetErrorString(e));
            return BQ_ERR_HIP;
        }
        return BQ_OK;
    }
};

extern "C" int bq_pairwise_coupling(bq_ctx *c, int ncls, int64_t t, const double *F, const double *A, const double *B, double *prob,
                                    int *iters, double *R) {
    BQ_TRY(couple_check(c, ncls, t, F, A, B, prob));
    BQ_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    couple_buffers buf;   // freed after the closing sync
    double *dF = nullptr;
    int rc = buf.alloc(ncls, t, A, B, R != nullptr, st);
    if (rc == BQ_OK) {
        dF = buf.mem.dev<double>(t * buf.P);
        hipError_t e = buf.mem.error();
        if (e == hipSuccess) e = hipMemcpyAsync(dF, F, sizeof(double) * t * buf.P, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) {
            bq_set_error("pairwise coupling setup failed: %s", hipGetErrorString(e));
            rc = e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
        }
    }
    if (rc == BQ_OK) rc = couple_launch(ncls, t, dF, buf.P, 1, buf.A, buf.B, buf.prob, buf.iters, buf.R, st);
    if (rc == BQ_OK) rc = buf.download(prob, iters, R, st);
    return bq_ctx_sync_after(c, rc);   // F, A, B and the results are the caller's
}

extern "C" int bq_decision_coupled(bq_ctx *c, int kernel, double gamma, double coef0, int degree, int64_t m, int64_t d,
                                   const double *SV, int k, const double *W, const double *b, int64_t t, const double *Xt, int ncls,
                                   const double *A, const double *B, double *prob, int *iters, double *R, double *dec) {
    BQ_ARG(SV && W && Xt, "NULL argument");
    BQ_TRY(couple_check(c, ncls, t, Xt, A, B, prob));
    BQ_ARG(m >= 1 && d >= 1, "m/d");
    BQ_ARG(k == ncls * (ncls - 1) / 2, "k must be the ncls (ncls - 1) / 2 pair columns");
    BQ_ARG(kernel != BQ_KERNEL_LAPLACIAN, "the Laplacian kernel has no GEMM form: bq_decision_function per column, then bq_pairwise_coupling");
    BQ_ARG(kernel == BQ_KERNEL_LINEAR || kernel == BQ_KERNEL_POLY || kernel == BQ_KERNEL_RBF || kernel == BQ_KERNEL_SIGMOID,
           "unknown kernel");
    BQ_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    couple_buffers buf;   // freed after the closing sync
    int rc = buf.alloc(ncls, t, A, B, R != nullptr, st);
    if (rc == BQ_OK) {
        // the decision values of a chunk of test points are coupled where the reduce kernel left them: column q of point i at
        // dout[q * t + i]
        struct call { couple_buffers *buf; int64_t t; hipStream_t st; } cl{&buf, t, st};
        rc = bq_launch_decision_multi(
            c, kernel, gamma, coef0, degree, m, d, SV, k, W, b, t, Xt, dec,
            [](void *arg, const double *dout, int64_t r0, int64_t r1) {
                const call *x = (const call *)arg;
                const couple_buffers &u = *x->buf;
                return couple_launch(u.k, r1 - r0, dout + r0, 1, x->t, u.A, u.B, u.prob + r0 * u.k, u.iters + r0,
                                     u.R ? u.R + r0 * u.P : nullptr, x->st);
            },
            &cl);
    }
    if (rc == BQ_OK) rc = buf.download(prob, iters, R, st);
    return bq_ctx_sync_after(c, rc);
}
