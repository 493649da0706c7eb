// The one copy of what closes every O(n) kernel of the single-problem solvers: wave ladder -> block tree -> one partial per block in
// global memory -> a ticket, so that the workgroup that arrives LAST finishes the reduction (strided by BQ_VEC_BLOCK, the same
// tree) and takes the scalar decisions in the same launch.  Every order is fixed, so a result does not depend on which workgroup is
// last, on the launch geometry or on the rank count.
//
// The hand-off (bq_last_block) is the only place that states the protocol:
//   1. lane 0 of the workgroup stores its partials (bq_part_put), the results of block reductions;
//   2. __syncthreads();
//   3. thread 0: __threadfence(), an explicit s_waitcnt vmcnt(0) lgkmcnt(0), the ticket's atomicAdd; the verdict goes to LDS;
//   4. __syncthreads();
//   5. the last workgroup: __threadfence(), thread 0 sets the ticket back to 0 for the next launch on the stream.
// The wait of step 3 is needed ALWAYS (MI355X_MICROARCH.md, "Compiler hazard (ROCm 7.2, gfx950)"): the compiler may drop the
// fence's own wait, and the ticket can then overtake the write-back of the partials.  Partials travel as agent-scope relaxed
// atomics, which stay correct whatever the acquire of step 5 does to the reader's L1; the last workgroup pays nblk / 256 such
// loads per thread.  tests/test_gpu_last_block.py checks every word of the hand-off under uneven load.
#pragma once
#include "bq_common.h"

// element i of this thread, item by item: block b owns [1024 b, 1024 (b + 1)), lane t the elements 1024 b + 256 j + t
#define BQ_VEC_LOOP(i)                                                          \
    const int64_t _base = (int64_t)blockIdx.x * BQ_VEC_TILE + threadIdx.x;      \
    _Pragma("unroll") for (int _j = 0; _j < BQ_VEC_ITEMS; ++_j)                 \
        for (int64_t i = _base + (int64_t)_j * BQ_VEC_BLOCK, _once = 1; _once; _once = 0)

static inline dim3 bq_vec_grid(int64_t ld) { return dim3((unsigned)(ld / BQ_VEC_TILE)); }

// ---- a wave: lane 0 receives the result ---------------------------------------------------------------------------------------
struct bq_op_sum {
    template <typename T>
    static __device__ __forceinline__ T f(T a, T b) { return a + b; }
};
struct bq_op_min {
    static __device__ __forceinline__ double f(double a, double b) { return fmin(a, b); }
    static __device__ __forceinline__ int f(int a, int b) { return min(a, b); }
};
struct bq_op_max {
    static __device__ __forceinline__ double f(double a, double b) { return fmax(a, b); }
};
template <typename OP, typename T>
__device__ __forceinline__ T bq_wave_reduce(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = OP::f(v, __shfl_down(v, off, 64));
    return v;
}
__device__ __forceinline__ double bq_wave_sum(double v) { return bq_wave_reduce<bq_op_sum>(v); }
__device__ __forceinline__ int bq_wave_sum(int v) { return bq_wave_reduce<bq_op_sum>(v); }
__device__ __forceinline__ double bq_wave_min(double v) { return bq_wave_reduce<bq_op_min>(v); }
__device__ __forceinline__ int bq_wave_min(int v) { return bq_wave_reduce<bq_op_min>(v); }
__device__ __forceinline__ double bq_wave_max(double v) { return bq_wave_reduce<bq_op_max>(v); }

// ---- a workgroup of WAVES waves -----------------------------------------------------------------------------------------------
// the waves' results in sh[0 .. WAVES): four are added ((0 + 1) + 2) + 3, sixteen in ascending order onto 0
template <int WAVES, typename T>
__device__ __forceinline__ T bq_waves_sum(const T *sh) {
    if constexpr (WAVES == 4) {
        return ((sh[0] + sh[1]) + sh[2]) + sh[3];
    } else {
        T r = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) r += sh[w];
        return r;
    }
}
template <int WAVES, typename T>
__device__ __forceinline__ T bq_waves_min(const T *sh) {
    T r = sh[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = bq_op_min::f(r, sh[w]);
    return r;
}
// Several quantities at once share one barrier pair: each goes through a row of its own (bq_wave_put: the wave's result into
// sh[wave], no barrier), the caller places ONE __syncthreads() and reads the rows with bq_waves_sum / bq_waves_min.
template <typename OP, typename T>
__device__ __forceinline__ void bq_wave_put(T v, T *sh) {
    v = bq_wave_reduce<OP>(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
}
// one quantity; every thread receives the result.  The barrier BEFORE the store makes back-to-back calls on the same sh safe
// (with the barrier after the read instead, the sixteen-wave users hold ten to sixteen registers more).
template <int WAVES = 4, typename T>
__device__ __forceinline__ T bq_block_sum(T v, T *sh) {
    v = bq_wave_reduce<bq_op_sum>(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return bq_waves_sum<WAVES>(sh);
}
template <int WAVES = 4, typename T>
__device__ __forceinline__ T bq_block_min(T v, T *sh) {
    v = bq_wave_reduce<bq_op_min>(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return bq_waves_min<WAVES>(sh);
}

// ---- a grid: partials, the ticket, the final reduction ------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void bq_part_put(T *part, T v) {
    __hip_atomic_store(part, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ T bq_part_get(const T *part) {
    return __hip_atomic_load(part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Called by ALL threads of a workgroup of any size, after lane 0 stored the workgroup's partials; `arrivals` workgroups take this
// ticket in the launch.  Every thread learns whether this workgroup arrived last; the ticket is 0 again when it has.
__device__ __forceinline__ bool bq_last_block(unsigned int *ticket, unsigned int arrivals) {
    __shared__ int last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        last = atomicAdd(ticket, 1u) == arrivals - 1 ? 1 : 0;
    }
    __syncthreads();
    if (!last) return false;
    __threadfence();
    if (threadIdx.x == 0) *ticket = 0u;
    return true;
}

// the last workgroup's sum / minimum over the nblk partials; threads 0 .. 255 of a 256-thread workgroup, every thread receives it
__device__ __forceinline__ double bq_final_sum(const double *part, int64_t nblk, double *sh) {
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < nblk; i += BQ_VEC_BLOCK) a += bq_part_get(&part[i]);
    return bq_block_sum(a, sh);
}
__device__ __forceinline__ double bq_final_min(const double *part, int64_t nblk, double *sh) {
    double a = INFINITY;
    for (int64_t i = threadIdx.x; i < nblk; i += BQ_VEC_BLOCK) a = fmin(a, bq_part_get(&part[i]));
    return bq_block_min(a, sh);
}
