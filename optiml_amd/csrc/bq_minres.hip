// MINRES on the normal equations of the restricted system — the active-set fallback for a singular Q[A,A].
//
// The reference catches the failed Cholesky and calls scipy.sparse.linalg.minres(Q_AA Q_AA^T, -(Q_AA^T q_A)) with its
// defaults (optiml/opti/constrained/active_set.py:142-151; scipy 1.15.3 here, unpinned in the reference): rtol 1e-5,
// maxiter 5 n, x0 = 0, no shift, no preconditioner.  This is a restatement of that Paige-Saunders iteration (Lanczos
// three-term recurrence + Givens rotations, the same stopping tests in the same order) as ONE persistent workgroup:
// the iteration is a strict chain of small matrix-vector products and scalar recurrences, so a single 1024-thread
// workgroup with the restricted Hessian resident in L2 avoids ~10 launches and 3 host round-trips per iteration.
// The operator is applied as H (H v) with the symmetric H = Q[A,A] instead of forming H H^T.
// Parity can only be loose: the singular case is decided by rounding in the reference as well.
#include <cstdlib>

#include "bq_chol.h"
#include "bq_minres_rec.h"
#include "bq_reduce.h"

constexpr int MT = 1024;   // threads of the persistent workgroup

__device__ __forceinline__ double mr_dot(const double *a, const double *b, int n, double *sh) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += MT) s = fma(a[i], b[i], s);
    return bq_block_sum<MT / 64>(s, sh);
}

// y = H x for the symmetric n x n matrix H (row pitch ld): one wave per row, lanes along the columns
__device__ __forceinline__ void mr_matvec(const double *__restrict__ H, int64_t ld, int n, const double *x, double *y) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int r = wv; r < n; r += MT / 64) {
        const double *row = H + (int64_t)r * ld;
        double s = 0.0;
        for (int c = lane; c < n; c += 64) s = fma(row[c], x[c], s);
        s = bq_wave_sum(s);
        if (lane == 0) y[r] = s;
    }
    __syncthreads();
}

// vec: 10 scratch vectors of length np.  rhs holds q' = -(q_A + ...) on entry and the solution on exit.
__global__ __launch_bounds__(MT) void minres_normal_kernel(const double *__restrict__ H, int64_t ld, const int *nA_ptr,
                                                           double *__restrict__ rhs, double *__restrict__ vec,
                                                           int64_t np, double rtol, int *__restrict__ iters) {
    __shared__ double sh[MT / 64];
    const int n = *nA_ptr;
    const int tid = threadIdx.x;
    // Ra/Rb/Rc rotate through the roles (r1, r2 = y, next Lanczos vector) of the three-term recurrence
    double *b = vec, *x = vec + np, *Ra = vec + 2 * np, *Rb = vec + 3 * np, *Rc = vec + 4 * np, *v = vec + 5 * np,
           *w = vec + 6 * np, *w1 = vec + 7 * np, *w2 = vec + 8 * np, *tmp = vec + 9 * np;
    const int maxiter = 5 * n;

    // b = H q'   (= -(Q_AA^T q_A));  x = 0;  r1 = b;  y = r1
    mr_matvec(H, ld, n, rhs, b);
    for (int i = tid; i < n; i += MT) {
        x[i] = 0.0;
        Ra[i] = b[i];
        w[i] = 0.0;
        w2[i] = 0.0;
    }
    __syncthreads();
    bq_minres_rec m;
    m.start(mr_dot(Ra, Ra, n, sh));
    int itn = 0;
    if (m.beta1 > 0.0) {   // beta1 == 0: the exact solution is x0 = 0 (also covers b == 0)
        double *r1p = Ra, *r2p = Ra, *y = Ra;   // r1 = b, r2 = r1, y = psolve(r1) = r1
        while (itn < maxiter) {
            itn += 1;
            const double s = 1.0 / m.beta;
            for (int i = tid; i < n; i += MT) v[i] = s * y[i];
            __syncthreads();
            mr_matvec(H, ld, n, v, tmp);     // operator = H H^T = H H
            double *ynew = (Ra != r1p && Ra != r2p) ? Ra : ((Rb != r1p && Rb != r2p) ? Rb : Rc);
            mr_matvec(H, ld, n, tmp, ynew);
            if (itn >= 2) {
                const double c = m.beta / m.oldb;
                for (int i = tid; i < n; i += MT) ynew[i] = ynew[i] - c * r1p[i];
                __syncthreads();
            }
            const double alfa = mr_dot(v, ynew, n, sh);
            {
                const double c = alfa / m.beta;
                for (int i = tid; i < n; i += MT) ynew[i] = ynew[i] - c * r2p[i];
                __syncthreads();
            }
            // r1 = r2; r2 = y; y = psolve(r2) = r2
            r1p = r2p;
            r2p = ynew;
            y = ynew;
            const double beta2 = mr_dot(r2p, y, n, sh);
            if (beta2 < 0.0) break;   // scipy's istop = 7
            m.rotate(alfa, beta2, itn);
            const double oldeps = m.oldeps, delta = m.delta, denom = m.denom, phi = m.phi;
            // w1 = w2; w2 = w; w = (v - oldeps*w1 - delta*w2) * denom; x += phi*w
            double *wold = w1;
            w1 = w2;
            w2 = w;
            w = wold;
            double xn = 0.0;
            for (int i = tid; i < n; i += MT) {
                const double wn = (v[i] - oldeps * w1[i] - delta * w2[i]) * denom;
                w[i] = wn;
                const double xi = x[i] + phi * wn;
                x[i] = xi;
                xn = fma(xi, xi, xn);
            }
            if (m.stop(bq_block_sum<MT / 64>(xn, sh), itn, maxiter, rtol) != 0) break;
        }
    }
    __syncthreads();
    for (int i = tid; i < (int)np; i += MT) rhs[i] = (i < n) ? x[i] : 0.0;
    if (tid == 0 && iters) *iters = itn;
}

// ---------------------------------------------------------------------------------------------------------------
// The same iteration for restricted systems of ANY size (the reference falls through to minres whatever |A| is,
// active_set.py:142-151): the two products H (H v) are HBM-streaming row-block kernels over all CUs, the O(n) updates are
// three fused vector kernels whose last-finishing block carries the scalar recurrences (Lanczos coefficients, Givens
// rotation, the stopping tests in scipy's order) in a device-resident state, reductions are fixed two-stage trees.  The
// host enqueues batches of iterations blind and looks at the `done` flag between batches; kernels early-exit on it.
// ---------------------------------------------------------------------------------------------------------------
struct mr_state {
    bq_minres_rec r;
    double rtol;
    long long itn, maxiter;
    int done;
    unsigned int ticket[4];
};

constexpr int MV_T = BQ_VEC_BLOCK;   // the vector kernels walk BQ_VEC_LOOP; np is a multiple of 128 only: `i < np` at every use
typedef double mr_d2 __attribute__((ext_vector_type(2)));

// y[r] = sum_c H[r][c] x[c], c < np (np a multiple of 128; rows are 16-byte aligned): one workgroup per 4 rows
__global__ __launch_bounds__(MV_T) void mr_gemv_kernel(const double *__restrict__ H, int64_t ld, int64_t np,
                                                       const double *__restrict__ x, double *__restrict__ y,
                                                       const mr_state *st) {
    if (st->done) return;
    constexpr int R = 4;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * R;
    double acc[R] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t c = 2 * (int64_t)tid; c < np; c += 2 * MV_T) {
        const mr_d2 xv = *reinterpret_cast<const mr_d2 *>(x + c);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = r0 + r < np ? r0 + r : np - 1;
            const mr_d2 h = *reinterpret_cast<const mr_d2 *>(H + row * ld + c);
            acc[r] = fma(h.y, xv.y, fma(h.x, xv.x, acc[r]));
        }
    }
    __shared__ double red[4][R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double s = bq_wave_sum(acc[r]);
        if (lane == 0) red[wv][r] = s;
    }
    __syncthreads();
    if (tid < R && r0 + tid < np) y[r0 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// partial -> part[block]; the block that takes the last ticket gets the total (fixed order), the others false
__device__ __forceinline__ bool mv_total(double local, double *part, unsigned int *ticket, double *sh, double *total) {
    const double b = bq_block_sum(local, sh);
    if (threadIdx.x == 0) bq_part_put(&part[blockIdx.x], b);
    if (!bq_last_block(ticket, gridDim.x)) return false;
    *total = bq_final_sum(part, gridDim.x, sh);
    return true;
}

// b = H q' is in Ra already: x = 0, w = w2 = 0, |b|^2 -> beta1 and the start values of the recurrences
__global__ __launch_bounds__(MV_T) void mr_init_kernel(int64_t np, const double *__restrict__ Ra, double *x, double *W0,
                                                       double *W2, double *part, mr_state *st, long long maxiter, double rtol) {
    __shared__ double sh[4];
    double s = 0.0;
    BQ_VEC_LOOP(i) {
        if (i < np) {
            x[i] = 0.0;
            W0[i] = 0.0;
            W2[i] = 0.0;
            s = fma(Ra[i], Ra[i], s);
        }
    }
    double tot;
    if (mv_total(s, part, &st->ticket[0], sh, &tot) && threadIdx.x == 0) {
        st->r.start(tot);   // the host zeroed the state (tickets, itn) before the first product
        st->maxiter = maxiter;
        st->rtol = rtol;
        st->done = tot > 0.0 ? 0 : 1;   // beta1 == 0: the exact solution is x0 = 0
    }
}

__global__ __launch_bounds__(MV_T) void mr_scale_kernel(int64_t np, const double *__restrict__ y, double *v, const mr_state *st) {
    if (st->done) return;
    const double s = 1.0 / st->r.beta;
    BQ_VEC_LOOP(i) {
        if (i < np) v[i] = s * y[i];
    }
}

// after ynew = H H v:  [ynew -= (beta / oldb) r1];  alfa = v . ynew
__global__ __launch_bounds__(MV_T) void mr_alfa_kernel(int64_t np, int sub_r1, const double *__restrict__ v, double *ynew,
                                                       const double *__restrict__ r1, double *part, mr_state *st) {
    if (st->done) return;
    __shared__ double sh[4];
    const double c = sub_r1 ? st->r.beta / st->r.oldb : 0.0;
    double s = 0.0;
    BQ_VEC_LOOP(i) {
        if (i < np) {
            double y = ynew[i];
            if (sub_r1) {
                y = y - c * r1[i];
                ynew[i] = y;
            }
            s = fma(v[i], y, s);
        }
    }
    double tot;
    if (mv_total(s, part, &st->ticket[1], sh, &tot) && threadIdx.x == 0) st->r.alfa = tot;
}

// ynew -= (alfa / beta) r2;  beta' = |ynew|;  the Givens rotation and everything scalar up to the solution update
__global__ __launch_bounds__(MV_T) void mr_beta_kernel(int64_t np, long long itn, double *ynew, const double *__restrict__ r2,
                                                       double *part, mr_state *st) {
    if (st->done) return;
    __shared__ double sh[4];
    const double c = st->r.alfa / st->r.beta;
    double s = 0.0;
    BQ_VEC_LOOP(i) {
        if (i < np) {
            const double y = ynew[i] - c * r2[i];
            ynew[i] = y;
            s = fma(y, y, s);
        }
    }
    double tot;
    if (mv_total(s, part, &st->ticket[2], sh, &tot) && threadIdx.x == 0) {
        bq_minres_rec r = st->r;
        r.rotate(r.alfa, tot, itn);
        st->r = r;
    }
}

// w = (v - oldeps w1 - delta w2) / gamma;  x += phi w;  |x| -> the stopping tests;  v <- ynew / beta for the next iteration
__global__ __launch_bounds__(MV_T) void mr_update_kernel(int64_t np, long long itn, double *v, const double *__restrict__ ynew,
                                                         double *w, const double *__restrict__ w1, const double *__restrict__ w2,
                                                         double *x, double *part, mr_state *st) {
    if (st->done) return;
    __shared__ double sh[4];
    const double oldeps = st->r.oldeps, delta = st->r.delta, denom = st->r.denom, phi = st->r.phi, beta = st->r.beta;
    const double nexts = beta > 0.0 ? 1.0 / beta : 0.0;
    double s = 0.0;
    BQ_VEC_LOOP(i) {
        if (i < np) {
            const double wn = (v[i] - oldeps * w1[i] - delta * w2[i]) * denom;
            w[i] = wn;
            const double xi = x[i] + phi * wn;
            x[i] = xi;
            s = fma(xi, xi, s);
            v[i] = nexts * ynew[i];
        }
    }
    double tot;
    if (mv_total(s, part, &st->ticket[3], sh, &tot) && threadIdx.x == 0) {
        st->itn = itn;
        if (st->r.stop(tot, itn, st->maxiter, st->rtol) != 0) {
            __threadfence();
            st->done = 1;
        }
    }
}

__global__ __launch_bounds__(MV_T) void mr_finish_kernel(int64_t np, const int *nA_ptr, const double *__restrict__ x, double *rhs,
                                                         const mr_state *st, int *iters) {
    const int n = *nA_ptr;
    BQ_VEC_LOOP(i) {
        if (i < np) rhs[i] = i < n ? x[i] : 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && iters) *iters = (int)st->itn;
}

static int minres_normal_big(bq_chol_ws *ws, const int *nA_dev, int64_t nA, int64_t np, double *vec, int *iters_dev) {
    hipStream_t stm = ws->ctx->stream;
    const unsigned vb = (unsigned)((np + BQ_VEC_TILE - 1) / BQ_VEC_TILE), gb = (unsigned)((np + 3) / 4);
    if (!ws->mr_state) {
        ws->mr_state = ws->mem.dev<char>(256);
        BQ_HIP(ws->mem.error());
        BQ_HIP(hipHostMalloc((void **)&ws->mr_flag, 2 * sizeof(int), hipHostMallocDefault));
    }
    if (ws->mr_part_cap < (int64_t)vb) {
        ws->mem.release(ws->mr_part);
        BQ_HIP(ws->mem.dev(&ws->mr_part, vb));
        ws->mr_part_cap = vb;
    }
    mr_state *st = (mr_state *)ws->mr_state;
    static_assert(sizeof(mr_state) <= 256, "mr_state");
    double *b = vec, *x = vec + np, *R[3] = {vec + 2 * np, vec + 3 * np, vec + 4 * np}, *v = vec + 5 * np,
           *W[3] = {vec + 6 * np, vec + 7 * np, vec + 8 * np}, *tmp = vec + 9 * np;
    (void)b;
    const long long maxiter = 5 * (long long)nA;
    BQ_HIP(hipMemsetAsync(st, 0, sizeof(mr_state), stm));   // done = 0 for the first product
    // b = H q' goes straight into R[0] (r1 = b, y = r1)
    mr_gemv_kernel<<<gb, MV_T, 0, stm>>>(ws->H, ws->ldh, np, ws->rhs, R[0], st);
    mr_init_kernel<<<vb, MV_T, 0, stm>>>(np, R[0], x, W[0], W[2], ws->mr_part, st, maxiter, 1e-5);
    mr_scale_kernel<<<vb, MV_T, 0, stm>>>(np, R[0], v, st);
    long long k = 0;
    int batch = 8;
    while (k < maxiter) {
        BQ_HIP(hipMemcpyAsync(ws->mr_flag, &st->done, sizeof(int), hipMemcpyDeviceToHost, stm));
        BQ_HIP(hipStreamSynchronize(stm));
        if (ws->mr_flag[0]) break;
        for (int q = 0; q < batch && k < maxiter; ++q) {
            ++k;
            double *ynew = R[k % 3], *r2 = R[(k + 2) % 3], *r1 = R[(k + 1) % 3];   // (k-1) mod 3, (k-2) mod 3
            mr_gemv_kernel<<<gb, MV_T, 0, stm>>>(ws->H, ws->ldh, np, v, tmp, st);      // operator = H H^T = H H
            mr_gemv_kernel<<<gb, MV_T, 0, stm>>>(ws->H, ws->ldh, np, tmp, ynew, st);
            mr_alfa_kernel<<<vb, MV_T, 0, stm>>>(np, k >= 2 ? 1 : 0, v, ynew, r1, ws->mr_part, st);
            mr_beta_kernel<<<vb, MV_T, 0, stm>>>(np, k, ynew, r2, ws->mr_part, st);
            mr_update_kernel<<<vb, MV_T, 0, stm>>>(np, k, v, ynew, W[k % 3], W[(k + 1) % 3], W[(k + 2) % 3], x, ws->mr_part, st);
        }
        if (batch < 64) batch *= 2;
    }
    mr_finish_kernel<<<vb, MV_T, 0, stm>>>(np, nA_dev, x, ws->rhs, st, iters_dev);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

// nA: |A| on the host.  Up to hook minres_big_min (default 4096) rows the single persistent workgroup is faster (no launches at
// all); beyond that — and for any size the one workgroup could not hold — the multi-workgroup form.
int bq_minres_normal(bq_chol_ws *ws, const int *nA_dev, int64_t nA, int64_t np, double *vec, int *iters_dev) {
    const long long big_min = (long long)bq_hook_value("minres_big_min", 4096.0);   // read per call: tests switch the form inside one process
    if (nA >= big_min) return minres_normal_big(ws, nA_dev, nA, np, vec, iters_dev);
    minres_normal_kernel<<<1, MT, 0, ws->ctx->stream>>>(ws->H, ws->ldh, nA_dev, ws->rhs, vec, np, 1e-5, iters_dev);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}
