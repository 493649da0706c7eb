// The (value, index, rider) picks of the row-based SMO solvers over a workgroup of RSMO_T threads, shared by bq_rsmo.hip and
// bq_mrsmo.hip: the total orders of bq_rsmo_step.h, so a result does not depend on how a scan was cut into pieces.
#pragma once
#include "bq_common.h"
#include "bq_rsmo_step.h"

constexpr int RSMO_T = 256;        // threads per workgroup = columns per workgroup (the slice)

// every thread receives the winner
struct rsmo_min_order {
    static __device__ __forceinline__ bool before(double va, long long ia, double vb, long long ib) { return bq_rsmo_min_before(va, ia, vb, ib); }
};
struct rsmo_max_order {
    static __device__ __forceinline__ bool before(double va, long long ia, double vb, long long ib) { return bq_rsmo_max_before(va, ia, vb, ib); }
};
struct rsmo_victim_order {
    static __device__ __forceinline__ bool before(long long va, long long ia, long long vb, long long ib) { return bq_rsmo_victim_before(va, ia, vb, ib); }
};
template <typename V>
struct rsmo_pick_smem {
    V v[RSMO_T / 64];
    long long i[RSMO_T / 64];
    double k[RSMO_T / 64];
};
template <typename ORDER, typename V>
__device__ __forceinline__ void rsmo_block_pick(V &v, long long &idx, double &rider, rsmo_pick_smem<V> &sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const V v2 = __shfl_down(v, off, 64);
        const long long i2 = __shfl_down(idx, off, 64);
        const double k2 = __shfl_down(rider, off, 64);
        if (ORDER::before(v2, i2, v, idx)) {
            v = v2;
            idx = i2;
            rider = k2;
        }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        sh.v[threadIdx.x >> 6] = v;
        sh.i[threadIdx.x >> 6] = idx;
        sh.k[threadIdx.x >> 6] = rider;
    }
    __syncthreads();
    v = sh.v[0];
    idx = sh.i[0];
    rider = sh.k[0];
#pragma unroll
    for (int w = 1; w < RSMO_T / 64; ++w)
        if (ORDER::before(sh.v[w], sh.i[w], v, idx)) {
            v = sh.v[w];
            idx = sh.i[w];
            rider = sh.k[w];
        }
}
