// Measurements of the device and of a problem's product on it: the time of the panel product, and the three probes (HBM streaming,
// fp64 MFMA, stream occupation) that give the roofline figures and the watchdog's test their yardsticks.
#include <algorithm>

#include "bq_common.h"
#include "bq_reduce.h"

extern "C" int bq_problem_time_matvec(bq_problem *p, int reps, double *mean_ms) {
    BQ_ARG(p && mean_ms && reps > 0, "argument");
    bq_ctx *c = p->ctx;
    BQ_HIP(hipSetDevice(c->device));
    hipEvent_t e0, e1;
    BQ_HIP(hipEventCreate(&e0));
    BQ_HIP(hipEventCreate(&e1));
    const bool prof = c->profiling;
    c->profiling = false;
    bq_seg_table tab;
    if (p->symmetric) bq_sym_seg_table(p, &tab);
    auto local = [&]() {
        if (p->streamed)
            return bq_stream_sym_product(c, p->stream_img, p->n, p->nb, tab, p->kernel, p->gamma, p->coef0, p->degree, p->add_one, p->w,
                                         p->s, 0, nullptr);
        return p->symmetric ? bq_launch_symv(c, bq_problem_panel(p), p->add_one, p->nb, tab, p->w, p->slab, p->s, nullptr)
                            : bq_launch_gemv(c, p->panel, p->storage, p->add_one, p->r1 - p->r0, p->ld, p->w,
                                             p->s + p->r0, nullptr);
    };
    int rc = local();  // warm
    hipEventRecord(e0, c->stream);
    for (int i = 0; rc == BQ_OK && i < reps; ++i) rc = local();
    hipEventRecord(e1, c->stream);
    hipError_t e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    c->profiling = prof;
    BQ_TRY(rc);
    BQ_HIP(e);
    *mean_ms = (double)ms / reps;
    return BQ_OK;
}

// ---------------------------------------------------------------------------------------------
// HBM streaming probe: what a plain read-only sweep and a device-to-device copy reach on this GPU, so that a roofline
// fraction can be quoted against the measured ceiling as well as the nominal 8 TB/s
// ---------------------------------------------------------------------------------------------
typedef double probe_d2 __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void probe_read_kernel(const probe_d2 *__restrict__ src, int64_t n2,
                                                         double *__restrict__ sink) {
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
        const probe_d2 v = __builtin_nontemporal_load(src + i);
        acc += v.x + v.y;
    }
    if (acc == 12345.678) *sink = acc;   // keeps the loads alive, practically never true
}

extern "C" int bq_ctx_probe_bandwidth(bq_ctx *c, int64_t bytes, int reps, double *read_gbs, double *copy_gbs) {
    BQ_ARG(c && read_gbs && copy_gbs, "NULL argument");
    BQ_ARG(bytes >= (1 << 20) && reps >= 1, "bytes >= 1 MiB, reps >= 1");
    BQ_HIP(hipSetDevice(c->device));
    bytes &= ~(int64_t)4095;
    bq_scratch mem;   // every exit below is behind an event or stream synchronisation
    double *a = mem.dev<double>((size_t)bytes / 8), *b = mem.dev<double>((size_t)bytes / 8);   // (bytes: a multiple of 4096)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = mem.error();
    if (e == hipSuccess) e = hipMemsetAsync(a, 0, (size_t)bytes, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(b, 0, (size_t)bytes, c->stream);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float ms_read = 0.f, ms_copy = 0.f;
    if (e == hipSuccess) {
        const int64_t n2 = bytes / 16;
        const unsigned grid = (unsigned)(c->num_cu * 16);
        probe_read_kernel<<<grid, 256, 0, c->stream>>>((const probe_d2 *)a, n2, b);   // warm
        hipEventRecord(e0, c->stream);
        for (int r = 0; r < reps; ++r) probe_read_kernel<<<grid, 256, 0, c->stream>>>((const probe_d2 *)a, n2, b);
        hipEventRecord(e1, c->stream);
        e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms_read, e0, e1);
    }
    if (e == hipSuccess) {
        hipMemcpyAsync(b, a, (size_t)bytes, hipMemcpyDeviceToDevice, c->stream);   // warm
        hipEventRecord(e0, c->stream);
        for (int r = 0; r < reps; ++r) hipMemcpyAsync(b, a, (size_t)bytes, hipMemcpyDeviceToDevice, c->stream);
        hipEventRecord(e1, c->stream);
        e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms_copy, e0, e1);
    }
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    if (e != hipSuccess) {
        bq_set_error("bandwidth probe failed: %s", hipGetErrorString(e));
        return BQ_ERR_HIP;
    }
    *read_gbs = (double)bytes * reps / (ms_read * 1e-3) / 1e9;
    *copy_gbs = 2.0 * (double)bytes * reps / (ms_copy * 1e-3) / 1e9;   // bytes read + bytes written
    return BQ_OK;
}

// ---------------------------------------------------------------------------------------------
// fp64 MFMA probe: what back-to-back v_mfma_f64_16x16x4_f64 with register operands sustain on this GPU at the clock it
// holds under that load — the yardstick beside the nominal 78.6 TFLOP/s for the Cholesky's roofline fraction
// ---------------------------------------------------------------------------------------------
typedef double probe_d4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256, 2) void probe_mfma_kernel(double *sink, int iters, double seed) {
    probe_d4 acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = (probe_d4){0.0, 0.0, 0.0, 0.0};
    double a = seed + 1e-3 * (double)(threadIdx.x & 15), b = 1.0 - 1e-3 * (double)(threadIdx.x >> 4);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
        a = -a;   // keeps the sums bounded without touching the MFMA stream's shape
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += acc[i].x + acc[i].y + acc[i].z + acc[i].w;
    if (s == 12345.678) *sink = s;   // keeps the MFMAs alive, practically never true
}

extern "C" int bq_ctx_probe_mfma_f64(bq_ctx *c, double seconds, double *tflops) {
    BQ_ARG(c && tflops, "NULL argument");
    BQ_ARG(seconds > 0.0 && seconds <= 10.0, "seconds in (0, 10]");
    BQ_HIP(hipSetDevice(c->device));
    bq_scratch mem;
    double *sink = mem.dev<double>(1);
    BQ_HIP(mem.error());
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    const int iters = 4096;
    const unsigned grid = (unsigned)(c->num_cu * 2);           // 2 workgroups of 4 waves per CU: two waves per SIMD
    const double flop_per_launch = (double)grid * 4.0 * iters * 16.0 * 2048.0;   // waves x iterations x MFMAs x 2*16*16*4
    float ms = 0.f;
    int launches = 0;
    if (e == hipSuccess) {
        // warm up for half the requested time so that the clock has settled under the load, then time the other half
        probe_mfma_kernel<<<grid, 256, 0, c->stream>>>(sink, iters, 0.5);
        hipEventRecord(e0, c->stream);
        probe_mfma_kernel<<<grid, 256, 0, c->stream>>>(sink, iters, 0.5);
        hipEventRecord(e1, c->stream);
        e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        const int per_half = ms > 0.f ? std::max(1, (int)(seconds * 500.0 / ms)) : 1;
        for (int i = 0; e == hipSuccess && i < per_half; ++i) probe_mfma_kernel<<<grid, 256, 0, c->stream>>>(sink, iters, 0.5);
        if (e == hipSuccess) {
            hipEventRecord(e0, c->stream);
            for (int i = 0; i < per_half; ++i) probe_mfma_kernel<<<grid, 256, 0, c->stream>>>(sink, iters, 0.5);
            hipEventRecord(e1, c->stream);
            e = hipEventSynchronize(e1);
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
            launches = per_half;
        }
    }
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    if (e != hipSuccess || ms <= 0.f) {
        bq_set_error("MFMA probe failed: %s", hipGetErrorString(e));
        return BQ_ERR_HIP;
    }
    *tflops = flop_per_launch * launches / (ms * 1e-3) / 1e12;
    return BQ_OK;
}

// ---------------------------------------------------------------------------------------------
// Stream occupancy probe (tests of the collective watchdog): ONE lane spins on the constant-rate wall clock for the given
// time and then returns — it always terminates by itself, whatever the host does
// ---------------------------------------------------------------------------------------------
__global__ void probe_stall_kernel(long long ticks, long long *sink) {
    const long long t0 = wall_clock64();
    long long t = t0;
    while (t - t0 < ticks) t = wall_clock64();
    if (ticks < 0) *sink = t;   // never: keeps the loop
}

extern "C" int bq_ctx_probe_stall(bq_ctx *c, double milliseconds, int behind_collective) {
    BQ_ARG(c != nullptr, "ctx is NULL");
    BQ_ARG(milliseconds > 0.0 && milliseconds <= 5000.0, "milliseconds in (0, 5000]");
    BQ_HIP(hipSetDevice(c->device));
    int rate_khz = 0;
    BQ_HIP(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, c->device));
    if (rate_khz <= 0) rate_khz = 100000;   // 100 MHz on every part this library is built for
    bq_scratch mem;
    double *one = nullptr;
    if (behind_collective) BQ_HIP(bq_dev_zeroed(hipSuccess, mem, &one, 1, c->stream));
    probe_stall_kernel<<<1, 1, 0, c->stream>>>((long long)(milliseconds * (double)rate_khz), nullptr);
    int rc = hipGetLastError() == hipSuccess ? BQ_OK : BQ_ERR_HIP;
    if (rc == BQ_OK && behind_collective) rc = bq_exchange_sum(c, one, 1);
    return bq_ctx_sync_after(c, rc);
}

// ---------------------------------------------------------------------------------------------
// The last-block hand-off of bq_reduce.h, checked word by word: `rounds` launches back to back on the stream, no host
// synchronisation between them.  In a launch block b puts one partial that depends on (b, round) and takes the ticket; the
// workgroup that arrives last compares EVERY partial with its expected word.  `uneven`: a block-dependent amount of ALU work
// first, so that the arrival order differs from the block order.  Every block first reads the partials of the previous round
// with plain loads (the consumer's L1 is warm with words that must NOT be seen again).  No block waits for another.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double probe_word(unsigned int b, int round) {
    return (double)(((unsigned long long)(b + 1u) << 20) | (unsigned long long)round);
}
__global__ __launch_bounds__(BQ_VEC_BLOCK) void probe_last_block_kernel(double *part, int round, int uneven, unsigned int *ticket,
                                                                        unsigned long long *bad) {
    const unsigned int b = blockIdx.x, nb = gridDim.x;
    double warm = 0.0;   // racing plain loads on purpose: the values are discarded, only the cache lines matter
    for (unsigned int i = threadIdx.x; i < nb; i += BQ_VEC_BLOCK) warm += part[i];
    asm volatile("" ::"v"(warm));
    if (uneven) {
        unsigned int h = b, spins = ((b * 2654435761u) >> 22) * 4u;   // 0 .. 4092 steps
        for (unsigned int k = 0; k < spins; ++k) h = h * 1664525u + 1013904223u;
        asm volatile("" ::"v"(h));
    }
    if (threadIdx.x == 0) bq_part_put(&part[b], probe_word(b, round));
    if (!bq_last_block(ticket, nb)) return;
    unsigned int wrong = 0;
    for (unsigned int i = threadIdx.x; i < nb; i += BQ_VEC_BLOCK) wrong += bq_part_get(&part[i]) != probe_word(i, round) ? 1u : 0u;
    if (wrong) atomicAdd(bad, (unsigned long long)wrong);
}

extern "C" int bq_ctx_probe_last_block(bq_ctx *c, int blocks, int rounds, int uneven, int64_t *bad_words, int *ticket_after) {
    BQ_ARG(c != nullptr && bad_words != nullptr && ticket_after != nullptr, "NULL argument");
    BQ_ARG(blocks >= 1 && blocks <= 65536, "blocks in [1, 65536]");
    BQ_ARG(rounds >= 1 && rounds <= 100000, "rounds in [1, 100000]");
    BQ_HIP(hipSetDevice(c->device));
    bq_scratch mem;
    double *part = nullptr;
    unsigned long long *state = nullptr;   // [0] mismatches, [1] the ticket (its low word)
    BQ_HIP(bq_dev_zeroed(hipSuccess, mem, &part, (size_t)blocks, c->stream));
    BQ_HIP(bq_dev_zeroed(hipSuccess, mem, &state, 2, c->stream));
    unsigned int *ticket = reinterpret_cast<unsigned int *>(state + 1);
    for (int r = 1; r <= rounds; ++r)
        probe_last_block_kernel<<<(unsigned)blocks, BQ_VEC_BLOCK, 0, c->stream>>>(part, r, uneven, ticket, state);
    int rc = hipGetLastError() == hipSuccess ? BQ_OK : BQ_ERR_HIP;
    unsigned long long host[2] = {0, 0};
    if (rc == BQ_OK && hipMemcpyAsync(host, state, sizeof(host), hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = BQ_ERR_HIP;
    rc = bq_ctx_sync_after(c, rc);
    if (rc != BQ_OK) return rc;
    *bad_words = (int64_t)host[0];
    *ticket_after = (int)(unsigned int)host[1];
    return BQ_OK;
}
