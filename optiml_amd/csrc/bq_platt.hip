// Batched Platt calibration: p = 1 / (1 + exp(A f + B)) fitted to (decision value, label) samples, the sigmoid of sklearn's
// CalibratedClassifierCV(method='sigmoid').  One 1024-thread workgroup per calibrator runs Newton's iteration with backtracking of
// Lin, Lin & Weng (2007) as libsvm's sigmoid_train states it: the targets (N+ + 1) / (N+ + 2) and 1 / (N- + 2), the start A = 0,
// B = log((N- + 1) / (N+ + 1)), sigma = 1e-12 on the Hessian's diagonal, the stop test |g_A|, |g_B| < 1e-5, the step halved while
// f_new >= f + 1e-4 step g'd down to 1e-10, at most 100 iterations.
//
// A calibrator reads its own row of D (decision values) and L (labels: > 0 positive, < 0 negative, 0 not in the sample: such a
// row enters no sum).  Every sum is taken as msvr_score_kernel (bq_mscore.hip) takes its sums: thread t adds the rows t, t + 1024,
// ... in ascending order, then a fixed tree over LDS; no atomics, nothing of another calibrator, so (A, B) have the same bits alone,
// at any position and in any batch.  Every thread reads the reduced values from LDS and so the whole workgroup takes every branch
// together; workgroups do not communicate.  The kernel is latency-bound (a handful of iterations over n values that stay in L2).
#include "bq_common.h"
#include "bq_scratch.h"

#include <cmath>

constexpr int PLATT_T = 1024;
constexpr int PLATT_MAX_ITER = 100;
constexpr double PLATT_MIN_STEP = 1e-10, PLATT_SIGMA = 1e-12, PLATT_EPS = 1e-5;

// the tree over the workgroup's 1024 partial sums of NV quantities; the totals go to res[0 .. NV), which every thread may read
// after the call.  Consecutive calls alternate between two `res` arrays: a thread that writes one of them again has passed the
// barriers of the call in between, which every thread reaches only after it has read the earlier totals, so no barrier is spent on
// protecting them.
template <int NV>
__device__ inline void platt_reduce(double (*s)[PLATT_T], double *res, const double *v, int tid) {
#pragma unroll
    for (int j = 0; j < NV; ++j) s[j][tid] = v[j];
    __syncthreads();
    for (int st = PLATT_T / 2; st > 1; st >>= 1) {
        if (tid < st) {
#pragma unroll
            for (int j = 0; j < NV; ++j) s[j][tid] += s[j][tid + st];
        }
        __syncthreads();
    }
    if (tid < NV) res[tid] = s[tid][0] + s[tid][1];
    __syncthreads();
}

// one sample's loss at z = A f + B with target t, in the form that overflows on neither side
__device__ inline double platt_loss_term(double z, double t) {
    return z >= 0.0 ? t * z + log1p(exp(-z)) : (t - 1.0) * z + log1p(exp(z));
}

__global__ __launch_bounds__(PLATT_T) void platt_fit_kernel(long long n, const double *__restrict__ D, const double *__restrict__ L,
                                                            double *__restrict__ A_out, double *__restrict__ B_out,
                                                            int *__restrict__ iters, double *__restrict__ loss,
                                                            long long *__restrict__ n_pos, long long *__restrict__ n_neg,
                                                            int *__restrict__ flags) {
    __shared__ double s[5][PLATT_T];
    __shared__ double res[2][5];
    const int tid = threadIdx.x;
    const long long cal = blockIdx.x;
    const double *f = D + cal * n, *lab = L + cal * n;
    int par = 0;
    double v[5];

    v[0] = v[1] = 0.0;   // the counts, exact in fp64
    for (long long i = tid; i < n; i += PLATT_T) {
        const double l = lab[i];
        v[0] += l > 0.0 ? 1.0 : 0.0;
        v[1] += l < 0.0 ? 1.0 : 0.0;
    }
    platt_reduce<2>(s, res[par], v, tid);
    const double np = res[par][0], nn = res[par][1];
    par ^= 1;
    if (np + nn == 0.0) {   // no labelled row: nothing to fit
        if (tid == 0) {
            A_out[cal] = 0.0;
            B_out[cal] = 0.0;
            iters[cal] = 0;
            loss[cal] = 0.0;
            n_pos[cal] = 0;
            n_neg[cal] = 0;
            flags[cal] = BQ_PLATT_EMPTY;
        }
        return;
    }
    const double hi = (np + 1.0) / (np + 2.0), lo = 1.0 / (nn + 2.0);

    auto loss_at = [&](double a, double b) {
        v[0] = 0.0;
        for (long long i = tid; i < n; i += PLATT_T) {
            const double l = lab[i];
            if (!(l > 0.0 || l < 0.0)) continue;
            v[0] += platt_loss_term(f[i] * a + b, l > 0.0 ? hi : lo);
        }
        platt_reduce<1>(s, res[par], v, tid);
        const double total = res[par][0];
        par ^= 1;
        return total;
    };

    double A = 0.0, B = log((nn + 1.0) / (np + 1.0));
    double fval = loss_at(A, B);
    int iter = 0, flag = 0;
    for (; iter < PLATT_MAX_ITER; ++iter) {
        v[0] = v[1] = v[2] = v[3] = v[4] = 0.0;
        for (long long i = tid; i < n; i += PLATT_T) {
            const double l = lab[i];
            if (!(l > 0.0 || l < 0.0)) continue;
            const double fi = f[i], z = fi * A + B, e = exp(-fabs(z));
            const double big = 1.0 / (1.0 + e), small = e / (1.0 + e);
            const double p = z >= 0.0 ? small : big, q = z >= 0.0 ? big : small;
            const double d2 = p * q, d1 = (l > 0.0 ? hi : lo) - p;
            v[0] += fi * fi * d2;
            v[1] += d2;
            v[2] += fi * d2;
            v[3] += fi * d1;
            v[4] += d1;
        }
        platt_reduce<5>(s, res[par], v, tid);
        const double h11 = res[par][0] + PLATT_SIGMA, h22 = res[par][1] + PLATT_SIGMA, h21 = res[par][2];
        const double g1 = res[par][3], g2 = res[par][4];
        par ^= 1;
        if (fabs(g1) < PLATT_EPS && fabs(g2) < PLATT_EPS) break;
        const double det = h11 * h22 - h21 * h21;
        const double dA = -(h22 * g1 - h21 * g2) / det, dB = -(-h21 * g1 + h11 * g2) / det;
        const double gd = g1 * dA + g2 * dB;
        double step = 1.0;
        bool moved = false;
        while (step >= PLATT_MIN_STEP) {
            const double newA = A + step * dA, newB = B + step * dB;
            const double newf = loss_at(newA, newB);
            if (newf < fval + 1e-4 * step * gd) {
                A = newA;
                B = newB;
                fval = newf;
                moved = true;
                break;
            }
            step *= 0.5;
        }
        if (!moved) {
            flag |= BQ_PLATT_LINE_SEARCH;
            break;
        }
    }
    if (iter >= PLATT_MAX_ITER) flag |= BQ_PLATT_MAX_ITER;
    if (tid == 0) {
        A_out[cal] = A;
        B_out[cal] = B;
        iters[cal] = iter;
        loss[cal] = fval;
        n_pos[cal] = (long long)np;
        n_neg[cal] = (long long)nn;
        flags[cal] = flag;
    }
}

int bq_launch_platt(int ncal, int64_t n, const double *D, const double *L, double *A, double *B, int *iters, double *loss,
                    long long *n_pos, long long *n_neg, int *flags, hipStream_t st) {
    platt_fit_kernel<<<(unsigned)ncal, PLATT_T, 0, st>>>((long long)n, D, L, A, B, iters, loss, n_pos, n_neg, flags);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

extern "C" int bq_platt_fit(bq_ctx *c, int ncal, int64_t n, const double *D, const double *L, double *A, double *B, int *iters,
                            double *loss, int64_t *n_pos, int64_t *n_neg, int *flags) {
    BQ_ARG(c && D && L && A && B && iters && loss && n_pos && n_neg && flags, "NULL argument");
    BQ_ARG(ncal >= 1, "ncal must be >= 1");
    BQ_ARG(n >= 1, "n must be >= 1");
    BQ_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    static_assert(sizeof(long long) == sizeof(int64_t), "the counts are copied as int64_t");
    const size_t len = (size_t)ncal * (size_t)n;
    bq_scratch mem;   // freed after the closing sync
    double *dD = mem.dev<double>(len), *dL = mem.dev<double>(len);
    double *dA = mem.dev<double>(ncal), *dB = mem.dev<double>(ncal), *dloss = mem.dev<double>(ncal);
    long long *dpos = mem.dev<long long>(ncal), *dneg = mem.dev<long long>(ncal);
    int *diters = mem.dev<int>(ncal), *dflags = mem.dev<int>(ncal);
    hipError_t e = mem.error();
    if (e == hipSuccess) e = hipMemcpyAsync(dD, D, sizeof(double) * len, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dL, L, sizeof(double) * len, hipMemcpyHostToDevice, st);
    int rc = BQ_OK;
    if (e != hipSuccess) {
        bq_set_error("Platt fit setup failed: %s", hipGetErrorString(e));
        rc = e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
    }
    if (rc == BQ_OK) rc = bq_launch_platt(ncal, n, dD, dL, dA, dB, diters, dloss, dpos, dneg, dflags, st);
    if (rc == BQ_OK) {
        e = hipMemcpyAsync(A, dA, sizeof(double) * ncal, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(B, dB, sizeof(double) * ncal, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(loss, dloss, sizeof(double) * ncal, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(n_pos, dpos, sizeof(int64_t) * ncal, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(n_neg, dneg, sizeof(int64_t) * ncal, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(iters, diters, sizeof(int) * ncal, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(flags, dflags, sizeof(int) * ncal, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) {
            bq_set_error("Platt fit: %s", hipGetErrorString(e));
            rc = BQ_ERR_HIP;
        }
    }
    return bq_ctx_sync_after(c, rc);   // D, L and the results are the caller's
}
