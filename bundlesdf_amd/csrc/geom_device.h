// Shared device helpers of the geometry kernels (cloud, nearest, ransac, pose_graph, mesh, mesh_smooth,
// texture, mesh_render): the rigid transform, the deterministic block sum, the rigid-fit sums, the
// pair-row clamp, the union-find walk and the uniform point grid. These kernels are held bit for bit
// against float64 oracles, and the bits depend on the order of operations stated here: a geometry
// kernel takes these from this header and does not restate them. All IEEE f64 without contraction;
// the pragma is the header's own, so including it before a file's pragma changes nothing.
#pragma once
#include "nof_device.h"

#pragma clang fp contract(off)

namespace nof {

// --- rigid transform ---------------------------------------------------------
// T: rows of [R | t], row stride 4 (a row-major 3x4 or the first 12 entries of a 4x4).
// out_k = ((T[k][0] x + T[k][1] y) + T[k][2] z) + T[k][3]; out may not alias T.
__device__ __forceinline__ void xform_point(const double *__restrict__ T, double x, double y, double z, double *out) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = ((T[k * 4] * x + T[k * 4 + 1] * y) + T[k * 4 + 2] * z) + T[k * 4 + 3];
}

// A direction (a normal): the rotation alone, out_k = (T[k][0] x + T[k][1] y) + T[k][2] z.
__device__ __forceinline__ void xform_dir(const double *__restrict__ T, double x, double y, double z, double *out) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = (T[k * 4] * x + T[k * 4 + 1] * y) + T[k * 4 + 2] * z;
}

// --- deterministic block sum -------------------------------------------------
// K per-lane values over the 256 threads of a block, no floating-point atomics: a butterfly (xor 32,
// 16, .. 1) adds the lanes of a wave, then the four waves are added in order through wave_sum, [4][K]
// of LDS. block_sum_waves leaves the wave sums in LDS behind a barrier, wave_total adds them for one k,
// and block_sum is the two together: thread k < K ends with total k in out[k]. Every thread of the
// block must call it.
template <int K>
__device__ __forceinline__ void block_sum_waves(double (&acc)[K], double (*wave_sum)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) wave_sum[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
}

template <int K>
__device__ __forceinline__ double wave_total(const double (*wave_sum)[K], int k) {
    return ((wave_sum[0][k] + wave_sum[1][k]) + wave_sum[2][k]) + wave_sum[3][k];
}

template <int K>
__device__ __forceinline__ void block_sum(double (&acc)[K], double (*wave_sum)[K], double *__restrict__ out) {
    block_sum_waves<K>(acc, wave_sum);
    if ((int)threadIdx.x < K) out[threadIdx.x] = wave_total<K>(wave_sum, threadIdx.x);
}

// --- rigid-fit sums ----------------------------------------------------------
// The sums evaluate._kabsch reads: [0] the count, [1..3] sum p, [4..6] sum t, [7..15] sum p t^T (row
// p, column t). Sum 16 is the caller's own (a squared distance of its choosing).
constexpr int RIGID_SUMS = 17;

__device__ __forceinline__ void rigid_moments_add(double (&acc)[RIGID_SUMS], const double *p, const double *t) {
    acc[0] += 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        acc[1 + a] += p[a];
        acc[4 + a] += t[a];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[7 + a * 3 + c] += p[a] * t[c];
    }
}

// The pair's rows [s, s + n), both ends clamped into [0, M] whatever pair_start holds.
__device__ __forceinline__ void pair_rows(const int32_t *__restrict__ pair_start, int32_t p, int64_t M, int64_t &s,
                                          int32_t &n) {
    int64_t a = pair_start[p], b = pair_start[p + 1];
    a = a < 0 ? 0 : (a > M ? M : a);
    b = b < a ? a : (b > M ? M : b);
    s = a;
    n = (int32_t)(b - a);
}

// --- union-find --------------------------------------------------------------
// Root of v: labels never exceed their index and only ever decrease, so the walk strictly descends
// (at most v steps) even while other lanes hook (atomicMin on a root) and compress; a label outside
// [0, r) ends it. The loads are relaxed atomics: other lanes write these words at the same moment.
// A compressing kernel stores the same way, and only where the root differs from the label's index.
__device__ __forceinline__ int32_t uf_find(const int32_t *labels, int32_t v) {
    int32_t r = v;
    for (;;) {
        const int32_t l = __hip_atomic_load(labels + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (l >= r || l < 0) return r;
        r = l;
    }
}

__device__ __forceinline__ void uf_compress(int32_t *labels, int32_t v) {
    const int32_t r = uf_find(labels, v);
    if (r != v) __hip_atomic_store(labels + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// --- uniform point grid (built by nof_point_grid_build) ------------------------
struct PointGrid {
    double org[3], cell;
    int32_t dims[3];
    const int32_t *start;      // [cells + 1] first point of each cell, x fastest
    const double *cpts;        // [n,3] the points in cell order
    const int32_t *ids;        // [n] their input indices
};

inline PointGrid point_grid(const double *origin, const int32_t *dims, double cell, const int32_t *start,
                            const double *cpts, const int32_t *ids) {
    PointGrid g;
    for (int a = 0; a < 3; ++a) {
        g.org[a] = origin[a];
        g.dims[a] = dims[a];
    }
    g.cell = cell;
    g.start = start;
    g.cpts = cpts;
    g.ids = ids;
    return g;
}

// The cell of p, clamped into the grid; the comparisons come before the cast, and a NaN gives cell 0.
__device__ __forceinline__ void grid_cell(const PointGrid &g, const double *p, int c[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double x = floor((p[a] - g.org[a]) / g.cell);
        c[a] = !(x >= 0) ? 0 : (x > g.dims[a] - 1 ? g.dims[a] - 1 : (int)x);
    }
}

}  // namespace nof
