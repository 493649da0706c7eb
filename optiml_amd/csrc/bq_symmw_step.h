// Pieces of the fp64-MFMA symmetric panel products (bq_symmw.hip: every tile for up to 16 columns; bq_symmp.hip: the class-routed
// one-vs-one product): the blocking constants, the 16-element step loads of a lane's row, the f64 MFMA and the wave-local LDS barrier.
#pragma once
#include "bq_symv_tile.h"

namespace bq_mfma {   // the two product files take these short names with a using-directive
constexpr int WJG = 4;     // tiles per strip
constexpr int CK = BQ_SYMMW_CK;
constexpr int TP = 72;     // pitch (doubles) of a wave's 16 x 64 transpose image; also its 16 x 64 reduction image (pitch RP)
constexpr int RP = 65;
constexpr int WP = 17;     // pitch of the W_J stage (256 rows x 16 slots)
static_assert(CK == 16, "the column chunk is the MFMA's N");
}  // namespace bq_mfma

typedef double d4_t __attribute__((ext_vector_type(4)));

// the 16 elements of lane l's row in a step: element t sits at column f(t, h) (h = l>>4) of the 64-column quarter
template <typename T> struct step_ld;
template <> struct step_ld<double> {
    struct raw { d2_t v[8]; };
    static __device__ __forceinline__ int f(int t, int h) { return 8 * (t >> 1) + 2 * h + (t & 1); }
    static __device__ __forceinline__ void load(const double *row, int h, raw &r) {
#pragma unroll
        for (int q = 0; q < 8; ++q) r.v[q] = __builtin_nontemporal_load(reinterpret_cast<const d2_t *>(row + 8 * q + 2 * h));
    }
    static __device__ __forceinline__ double get(const raw &r, int t) { return (t & 1) ? r.v[t >> 1].y : r.v[t >> 1].x; }
};
template <> struct step_ld<bq_c7> {   // the compact layout: the fp64 columns, decoded at load
    struct raw { d2_t v[8]; };
    static __device__ __forceinline__ int f(int t, int h) { return step_ld<double>::f(t, h); }
    static __device__ __forceinline__ void load(const bq_c7p &row, int h, raw &r) {
#pragma unroll
        for (int q = 0; q < 8; ++q) r.v[q] = row.pair(8 * q + 2 * h);
    }
    static __device__ __forceinline__ double get(const raw &r, int t) { return (t & 1) ? r.v[t >> 1].y : r.v[t >> 1].x; }
};
template <> struct step_ld<float> {
    struct raw { f4_t v[4]; };
    static __device__ __forceinline__ int f(int t, int h) { return 16 * (t >> 2) + 4 * h + (t & 3); }
    static __device__ __forceinline__ void load(const float *row, int h, raw &r) {
#pragma unroll
        for (int q = 0; q < 4; ++q) r.v[q] = __builtin_nontemporal_load(reinterpret_cast<const f4_t *>(row + 16 * q + 4 * h));
    }
    static __device__ __forceinline__ double get(const raw &r, int t) { return (double)r.v[t >> 2][t & 3]; }
};

__device__ __forceinline__ d4_t mfma64(double a, double b, d4_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// the lanes of one wave exchange data through LDS between these
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
