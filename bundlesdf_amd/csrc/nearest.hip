// Exact nearest-neighbour search in a uniform cell grid, and the correspondence
// sums of one point-to-point ICP step: the device side of the run evaluation
// (benchmark_ho3d.py:18-139 with Utils.py:82-103,268-273 — ADD-S, chamfer and
// the registration before it, cKDTree / open3d there).
//
//  k_nearest       one thread per (transform, query): the query is moved by its
//                  transform, its clamped cell is searched, then the block of
//                  searched cells grows ring by ring; a ring's new cells are
//                  whole x-rows (contiguous in cell_start, one point range) above,
//                  below and beside the old block, and the two end cells of the
//                  rows that cross it. The search stops when no unsearched cell
//                  can hold a point as close as the best one (see face_gap), when
//                  every unsearched cell is beyond max_dist, or when the block
//                  covers the grid. The answer is the lowest input index among
//                  the points of smallest d2, so it does not depend on the order
//                  cells or points are visited in.
//  k_corr_moments  per block, in a fixed thread -> element assignment, the 17 sums
//                  of the matched pairs (n, sum p', sum q, sum p' q^T, sum dist^2):
//                  butterfly over the wave, waves added in order, one partial row
//                  per block; k_corr_final adds the rows in block order. No
//                  floating-point atomics: two runs give the same bits.
#include "geom_device.h"

#pragma clang fp contract(off)

namespace nof {

// Lower bound of |p_a - q_a| over the points p whose cell index along an axis is
// beyond the face at org + k cell, given g = the query's signed distance to that
// face (positive: the face is ahead). A point's cell comes from floor((p - org) /
// cell) in floating point, so it may lie a few ulps of the coordinate magnitude
// on the near side of the face: 1e-12 of that magnitude is taken off (thousands
// of ulps), and a face the query lies beyond (g <= 0) gives 0.
__device__ __forceinline__ double face_gap(double g, double magnitude) {
    const double s = g - 1e-12 * magnitude;
    return s > 0.0 ? s : 0.0;
}

__global__ __launch_bounds__(256) void k_nearest(PointGrid g, double max_dist, const double *__restrict__ queries,
                                                 int32_t Q, const double *__restrict__ xforms,
                                                 int32_t *__restrict__ index, double *__restrict__ dist) {
    const int32_t qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= Q) return;
    const int32_t b = blockIdx.y;
    double q[3] = {queries[(size_t)qi * 3], queries[(size_t)qi * 3 + 1], queries[(size_t)qi * 3 + 2]};
    if (xforms) xform_point(xforms + (size_t)b * 16, q[0], q[1], q[2], q);
    int c[3];
    grid_cell(g, q, c);
    double best = __longlong_as_double(0x7ff0000000000000ll);
    int32_t bi = -1;
    auto scan = [&](int64_t first, int64_t last) {   // the points of cells first..last (one x-row piece)
        const int32_t e = g.start[last + 1];
        for (int32_t i = g.start[first]; i < e; ++i) {
            const double dx = g.cpts[(size_t)i * 3] - q[0], dy = g.cpts[(size_t)i * 3 + 1] - q[1],
                         dz = g.cpts[(size_t)i * 3 + 2] - q[2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 <= best) {
                const int32_t id = g.ids[i];
                if (d2 < best || id < bi) { best = d2; bi = id; }
            }
        }
    };
    for (int r = 0;; ++r) {
        int lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = c[a] - r > 0 ? c[a] - r : 0;
            hi[a] = c[a] + r < g.dims[a] - 1 ? c[a] + r : g.dims[a] - 1;   // c + r <= 2^27: no overflow
        }
        for (int z = lo[2]; z <= hi[2]; ++z) {
            const bool zin = r > 0 && z > c[2] - r && z < c[2] + r;
            for (int y = lo[1]; y <= hi[1]; ++y) {
                const int64_t row = ((int64_t)z * g.dims[1] + y) * g.dims[0];
                if (zin && y > c[1] - r && y < c[1] + r) {     // the row crosses the searched block
                    if (c[0] - r >= 0) scan(row + c[0] - r, row + c[0] - r);
                    if (c[0] + r <= g.dims[0] - 1) scan(row + c[0] + r, row + c[0] + r);
                } else {
                    scan(row + lo[0], row + hi[0]);
                }
            }
        }
        bool covered = true;
        double gap = __longlong_as_double(0x7ff0000000000000ll);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double mag = (fabs(g.org[a]) + fabs(q[a])) + (double)g.dims[a] * g.cell;
            if (lo[a] > 0) {
                covered = false;
                const double f = face_gap(q[a] - (g.org[a] + (double)lo[a] * g.cell), mag);
                gap = f < gap ? f : gap;
            }
            if (hi[a] < g.dims[a] - 1) {
                covered = false;
                const double f = face_gap((g.org[a] + (double)(hi[a] + 1) * g.cell) - q[a], mag);
                gap = f < gap ? f : gap;
            }
        }
        if (covered || best <= gap * gap || (max_dist > 0 && gap > max_dist)) break;
    }
    double d = sqrt(best);
    if (bi < 0 || (max_dist > 0 && d > max_dist)) {
        bi = -1;
        d = __longlong_as_double(0x7ff0000000000000ll);
    }
    index[(size_t)b * Q + qi] = bi;
    dist[(size_t)b * Q + qi] = d;
}

constexpr int MOMENT_BLOCKS = 1024;

__global__ __launch_bounds__(256) void k_corr_moments(const double *__restrict__ src, int32_t n,
                                                      const double *__restrict__ xform, const double *__restrict__ tgt,
                                                      int32_t m, const int32_t *__restrict__ index,
                                                      const double *__restrict__ dist, double *__restrict__ partial) {
    __shared__ double wave_sum[4][RIGID_SUMS];
    double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    if (xform) {
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = xform[k];
    }
    double acc[RIGID_SUMS];
#pragma unroll
    for (int k = 0; k < RIGID_SUMS; ++k) acc[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int32_t j = index[i];
        if (j < 0 || j >= m) continue;
        double p[3];
        xform_point(T, src[i * 3], src[i * 3 + 1], src[i * 3 + 2], p);
        rigid_moments_add(acc, p, tgt + (size_t)j * 3);
        acc[16] += dist[i] * dist[i];
    }
    block_sum<RIGID_SUMS>(acc, wave_sum, partial + (size_t)blockIdx.x * RIGID_SUMS);
}

__global__ __launch_bounds__(64) void k_corr_final(const double *__restrict__ partial, int32_t n_blocks,
                                                   double *__restrict__ out) {
    if (threadIdx.x >= RIGID_SUMS) return;
    double s = 0.0;
    for (int32_t b = 0; b < n_blocks; ++b) s += partial[(size_t)b * RIGID_SUMS + threadIdx.x];
    out[threadIdx.x] = s;
}

static int32_t moment_blocks(int32_t n) {
    const uint32_t nb = div_up((uint64_t)(n > 0 ? n : 1), 256);
    return (int32_t)(nb < (uint32_t)MOMENT_BLOCKS ? nb : (uint32_t)MOMENT_BLOCKS);
}

}  // namespace nof

using namespace nof;

extern "C" {

int nof_nearest_points(const double *queries, int32_t Q, const double *xforms, int32_t B, const int32_t *cell_start,
                       const double *cell_points, const int32_t *cell_ids, int32_t n, const double *origin,
                       const int32_t *dims, double cell, double max_dist, int32_t *index, double *dist, void *stream) {
    if (Q < 0 || B < 0 || n < 0) return set_error(NOF_EINVAL, "nearest_points: negative size (Q=%d, B=%d, n=%d)", Q, B, n);
    if (!xforms && B != 1) return set_error(NOF_EINVAL, "nearest_points: B=%d without transforms (NULL means B = 1)", B);
    if (B > 65535) return set_error(NOF_EINVAL, "nearest_points: B=%d transforms (max 65535)", B);
    if (!origin || !dims || !(cell > 0) || !cell_start || max_dist != max_dist)
        return set_error(NOF_EINVAL, "nearest_points: bad grid arguments");
    if (dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0) return set_error(NOF_EINVAL, "nearest_points: bad grid dims");
    const int64_t nc = (int64_t)dims[0] * dims[1] * dims[2];
    if (nc > (1ll << 26)) return set_error(NOF_EINVAL, "nearest_points: %lld grid cells (max 2^26)", (long long)nc);
    if (Q == 0 || B == 0) return 0;
    if (n == 0) return set_error(NOF_EINVAL, "nearest_points: empty cloud with %d queries", Q);
    if (!queries || !cell_points || !cell_ids || !index || !dist)
        return set_error(NOF_EINVAL, "nearest_points: NULL input/output pointer (cell_ids is required)");
    hipLaunchKernelGGL(k_nearest, dim3(div_up(Q, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       point_grid(origin, dims, cell, cell_start, cell_points, cell_ids), max_dist, queries, Q, xforms,
                       index, dist);
    return check_launch("nearest_points");
}

size_t nof_nearest_workspace_bytes(int32_t n) { return (size_t)moment_blocks(n) * RIGID_SUMS * sizeof(double); }

int nof_correspondence_moments(const double *source, int32_t n, const double *xform, const double *target, int32_t m,
                               const int32_t *index, const double *dist, double *sums, void *workspace, void *stream) {
    if (n < 0 || m < 0) return set_error(NOF_EINVAL, "correspondence_moments: negative size (n=%d, m=%d)", n, m);
    if (!sums || !workspace || (n > 0 && (!source || !index || !dist)) || (n > 0 && m > 0 && !target))
        return set_error(NOF_EINVAL, "correspondence_moments: NULL input/output pointer");
    const int32_t nb = n > 0 ? moment_blocks(n) : 0;
    if (nb > 0)
        hipLaunchKernelGGL(k_corr_moments, dim3(nb), dim3(256), 0, (hipStream_t)stream, source, n, xform, target, m,
                           index, dist, (double *)workspace);
    hipLaunchKernelGGL(k_corr_final, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double *)workspace, nb, sums);
    return check_launch("correspondence_moments");
}

}  // extern "C"
