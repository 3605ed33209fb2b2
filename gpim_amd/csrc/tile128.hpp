// tile128.hpp -- device-side pieces shared by the kernels that walk an N x N matrix in 128 x 128 tiles, one workgroup of
// 256 threads per tile (engine.hip: the covariance builds; grad.hip: the gradient contractions; predict.hip: leave-one-out):
// the fixed-shape reductions, the tile index, the staging of a tile's points into LDS and the gradient tile's epilogue.
// Every sum has one fixed order, so results are bit-reproducible run to run.
#pragma once
#include "common.hpp"

typedef double d2 __attribute__((ext_vector_type(2)));
typedef float f2 __attribute__((ext_vector_type(2)));
// The N x N matrices (covariance, factor, inverse, K* slab) are double or float (gpimhip_set_precision); vectors,
// reductions and every scalar stay double.  Host-side the pointers are typed double* for both.
template <typename R> struct Vec2;
template <> struct Vec2<double> { typedef d2 T; };
template <> struct Vec2<float> { typedef f2 T; };

__device__ __forceinline__ double wave_sum(double v) {
    v += __shfl_xor(v, 32);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}
// the sum over a workgroup of 256 threads (red: 256 doubles of LDS), valid in every thread
__device__ inline double block_sum_256(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
// Entry j of a vector that exists as row-chunk partial sums part[chunk][j] (engine.hip: gemv_t_tri_kernel; predict.hip:
// colsq_tri_kernel -- nR chunks of rc rows of a lower-triangular matrix of order np): the chunks at or below the
// column's diagonal block, in increasing order.
__device__ __forceinline__ double gemv_tri_alpha(const double* __restrict__ part, int nR, int rc, int64_t np, int64_t j) {
    double t = 0.0;
    for (int r = (int)(((j / NB) * NB) / rc); r < nR; ++r) t += part[(int64_t)r * np + j];
    return t;
}

// ---- tile index: workgroup q of a launch over the lower tiles (row by row), or over all tiles of ntc columns
__device__ __forceinline__ void lower_tile_from_linear(int q, int& i, int& j) {
    i = (int)((sqrt(8.0 * (double)q + 1.0) - 1.0) * 0.5);
    while ((int64_t)i * (i + 1) / 2 > q) --i;
    while ((int64_t)(i + 1) * (i + 2) / 2 <= q) ++i;
    j = q - (int)((int64_t)i * (i + 1) / 2);
}
__device__ __forceinline__ void tile_from_linear(int q, int ntc, bool lower, int& ci, int& cj) {
    if (lower) lower_tile_from_linear(q, ci, cj);
    else { ci = q / ntc; cj = q % ntc; }
}

// ---- staging.  Thread tid of the workgroup of tile (ci, cj) stages ONE point: threads 0 .. 127 row point ci * 128 + tid
// of X (N points), threads 128 .. 255 column point cj * 128 + tid - 128 of Z (M points).
struct TileSlot {
    bool isrow; int loc;        // which of the two LDS arrays, and the position in it
    int64_t g;                  // the point
    bool valid;                 // inside the matrix (the rest is padding)
};
// The point's coordinates over the lengthscales into xa (rows) / xz (columns), zeros for padding and unused dimensions;
// W == 5: the squared norm in slot 4 (the dense kernels' r2 = |a|^2 - 2 a.b + |b|^2), W == 4: coordinates only (the
// reflection kernels take differences).  Returns the slot: the caller stages what else it needs per point with tile_put.
// The caller's __syncthreads() ends the staging.
template <int W>
__device__ __forceinline__ TileSlot tile_stage(const double* __restrict__ X, int64_t N, const double* __restrict__ Z, int64_t M,
                                               int d, const ThetaDev& t, int ci, int cj, double (*xa)[W], double (*xz)[W]) {
    static_assert(W == GPIMHIP_MAX_DIM || W == GPIMHIP_MAX_DIM + 1, "coordinates, or coordinates and squared norm");
    const int tid = threadIdx.x;
    TileSlot s;
    s.isrow = tid < 128;
    s.loc = tid & 127;
    s.g = (int64_t)(s.isrow ? ci : cj) * 128 + s.loc;
    s.valid = s.g < (s.isrow ? N : M);
    const double* src = s.isrow ? X : Z;
    double (*dst)[W] = s.isrow ? xa : xz;
    double s2 = 0.0;
#pragma unroll
    for (int k = 0; k < GPIMHIP_MAX_DIM; ++k) {
        double a = 0.0;
        if (k < d && s.valid) a = src[s.g * d + k] / t.ls[k];
        dst[s.loc][k] = a;
        s2 += a * a;
    }
    if (W == GPIMHIP_MAX_DIM + 1) dst[s.loc][GPIMHIP_MAX_DIM] = s2;
    return s;
}
// a per-point value (alpha, weight) next to the coordinates
__device__ __forceinline__ void tile_put(const TileSlot& s, double* rows, double* cols, double v) { (s.isrow ? rows : cols)[s.loc] = v; }

// ---- epilogue of a gradient tile.  The seven sums S[] of every thread -> wave sums -> red[wave][k] -> threads 0 .. 7 add the
// four waves as (0 + 1) + (2 + 3) and store part_tile[k] (slot 7 = 0).
// COHERENT: the reader is another workgroup of the SAME launch, possibly on another XCD whose L2 is not coherent with this
// one: agent-scope (write-through, sc1) stores, and the storing wave then waits until they have been written (s_waitcnt
// vmcnt(0)) -- whatever the caller signals behind its next barrier cannot become visible before them.  A release FENCE instead
// (__threadfence: write back + invalidate the whole L2, once per workgroup) was measured at 1.87 ms for the launch at
// N = 16384 (0.40 without).
template <bool COHERENT>
__device__ __forceinline__ void tile_sums_store(const double* S, double (*red)[8], double* part_tile) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const double v = wave_sum(S[k]);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (tid < 8) {
        double v = 0.0;
        if (tid < 7) v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        if (COHERENT) __hip_atomic_store(part_tile + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else part_tile[tid] = v;
    }
    if (COHERENT && wave == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
