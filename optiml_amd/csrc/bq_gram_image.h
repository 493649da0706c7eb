// What the kernels that form Gram tiles from two row-major matrices share (bq_gram.hip: the panel build, the single-column
// decision function and the streamed product; bq_decide.hip: the fused multi-column decision function): the k-major, zero-padded
// image of a matrix with its squared row norms, and the kernel maps of the tile epilogue.  Everything here is static: each
// translation unit that includes it has its own copy.
#pragma once
#include "bq_common.h"
#include "bq_mfma_tile.h"

static __global__ void transpose_pad_kernel(const double *__restrict__ X, int64_t n, int64_t d, double *__restrict__ Xt,
                                     int64_t np, int64_t dp) {
    __shared__ double tile[32][33];
    const int64_t r0 = (int64_t)blockIdx.x * 32, k0 = (int64_t)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int j = ty; j < 32; j += 8) {
        int64_t r = r0 + j, k = k0 + tx;
        tile[j][tx] = (r < n && k < d) ? X[r * d + k] : 0.0;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        int64_t k = k0 + j, r = r0 + tx;
        if (k < dp && r < np) Xt[k * np + r] = tile[tx][j];
    }
}

static __global__ void row_norms_kernel(const double *__restrict__ X, int64_t n, int64_t d, double *__restrict__ out,
                                 int64_t np) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    double s = 0.0;
    if (i < n) {
        const double *row = X + i * d;
        for (int64_t k = 0; k < d; ++k) s = fma(row[k], row[k], s);
    }
    out[i] = s;
}

// (gamma <x, y> + coef0)^degree: degrees 2 and 3 (the reference's default) by multiplication — pow() is ~150 vector
// instructions per element, x * x * x two; <= 1 ulp from the reference's pow(x, 3.0).  DEG = 0: any degree, pow().  DEG = 1: x
// itself, as the reference's x ** 1 — the device's pow(x, 1.0) is not x for every x; an instantiation, not a test of `degree`
// beside pow(), which spilled (decide_multi_kernel<POLY, 1, 0>: 79 VGPRs, gram_stream_sym_kernel<POLY>: 213).
template <int DEG>
__device__ __forceinline__ double bq_poly_map(double x, int degree) {
    if (DEG == 1) return x;
    if (DEG == 2) return x * x;
    if (DEG == 3) return x * x * x;
    return pow(x, (double)degree);
}
#define BQ_EXP_ATTR __device__ __forceinline__
#define BQ_EXP_LOINT(t) __double2loint(t)
#include "bq_exp.h"

struct gram_images {
    bq_buffers<2> mem;   // At and a2: freed with the image, which a call declares after its bq_scratch and lets go behind its closing sync
    double *At = nullptr, *a2 = nullptr;
    int64_t mp = 0, dp = 0;
};

static int make_image(bq_ctx *ctx, const double *Xdev, int64_t n, int64_t d, gram_images *img) {
    img->mp = bq_round_up(n, BQ_GT);
    img->dp = bq_round_up(d, BQ_GK);
    img->At = img->mem.dev<double>(img->mp * img->dp);
    img->a2 = img->mem.dev<double>(img->mp);
    BQ_HIP(img->mem.error());
    dim3 grid((unsigned)((img->mp + 31) / 32), (unsigned)((img->dp + 31) / 32));
    transpose_pad_kernel<<<grid, 256, 0, ctx->stream>>>(Xdev, n, d, img->At, img->mp, img->dp);
    row_norms_kernel<<<(unsigned)((img->mp + 255) / 256), 256, 0, ctx->stream>>>(Xdev, n, d, img->a2, img->mp);
    BQ_HIP(hipGetLastError());
    return BQ_OK;
}

