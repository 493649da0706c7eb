// bq_ovo_vote: the one-vs-one vote of t rows of pair decision values (bq_vote.h: one thread per row, one wavefront per workgroup) —
// what OneVsOneSVC.predict does on the host with ovo_decision and argmax, as one launch.  The held-out scoring of a one-vs-one search
// (bq_msolver_pairs_vote_heldout, bq_mscore.hip) runs the same device function on the solver's own product.
#include "bq_vote.h"
#include "bq_scratch.h"

// D: t x P row-major; pred: t; Y: t x ncls or null
__global__ __launch_bounds__(BQ_VOTE_ROWS) void ovo_vote_kernel(int ncls, long long t, const double *__restrict__ D,
                                                                int *__restrict__ pred, double *__restrict__ Y) {
    extern __shared__ double vote_lds[];
    const long long i = (long long)blockIdx.x * BQ_VOTE_ROWS + threadIdx.x;
    if (i >= t) return;   // (no barrier follows: a lane's LDS column is its own)
    const long long P = (long long)ncls * (ncls - 1) / 2;
    const double *row = D + i * P;
    pred[i] = bq_ovo_vote_row(ncls, [row](int k) { return row[k]; }, vote_lds, (int)threadIdx.x, Y ? Y + i * ncls : nullptr);
}

extern "C" int bq_ovo_vote(bq_ctx *c, int ncls, int64_t t, const double *D, int *pred, double *Y) {
    BQ_ARG(c && D && pred, "NULL argument");
    BQ_ARG(ncls >= 2, "ncls must be >= 2");
    BQ_ARG(ncls <= BQ_VOTE_MAX_CLS, "the one-vs-one vote takes at most 64 classes");
    BQ_ARG(t >= 1, "t must be >= 1");
    BQ_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int64_t P = (int64_t)ncls * (ncls - 1) / 2;
    bq_scratch mem;   // freed after the closing sync
    double *dD = mem.dev<double>(t * P), *dY = Y ? mem.dev<double>(t * ncls) : nullptr;
    int *dpred = mem.dev<int>(t);
    hipError_t e = mem.error();
    if (e == hipSuccess) e = hipMemcpyAsync(dD, D, sizeof(double) * t * P, hipMemcpyHostToDevice, st);
    int rc = BQ_OK;
    if (e != hipSuccess) {
        bq_set_error("one-vs-one vote setup failed: %s", hipGetErrorString(e));
        rc = e == hipErrorOutOfMemory ? BQ_ERR_NOMEM : BQ_ERR_HIP;
    }
    if (rc == BQ_OK) {
        const unsigned blocks = (unsigned)((t + BQ_VOTE_ROWS - 1) / BQ_VOTE_ROWS);
        ovo_vote_kernel<<<blocks, BQ_VOTE_ROWS, bq_vote_lds_bytes(ncls), st>>>(ncls, (long long)t, dD, dpred, dY);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(pred, dpred, sizeof(int) * t, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && Y) e = hipMemcpyAsync(Y, dY, sizeof(double) * t * ncls, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) {
            bq_set_error("one-vs-one vote: %s", hipGetErrorString(e));
            rc = BQ_ERR_HIP;
        }
    }
    return bq_ctx_sync_after(c, rc);   // D and the results are the caller's
}
