// Mesh extraction on the device: the marching cubes of
// NerfRunner.extract_mesh (nerf_runner.py:1349-1408, skimage there) and the connected
// components of trimesh_split / largest_component (Utils.py:287-298, bundlesdf.py:748-759).
// Both reproduce bundlesdf_amd/mesh.py bit for bit and in the same order (DESIGN.md "Mesh
// extraction on the device" has the ordering argument).
//
//  k_mc_count      one lane per grid point, k fastest: the point's inside bit, the crossings of
//                  the three grid edges it owns (q, q + e_a), the case of the cell whose lowest
//                  corner it is and that case's triangle count. An exclusive scan over the block
//                  (wave shuffles, then the four wave totals through LDS) turns the two counts
//                  into block-local offsets; one 32-bit word per point keeps them with the
//                  crossing mask and the case. Per block: the two totals and the value range.
//  k_mc_vertices   one lane per grid point: its up to three vertices at
//                  block base + local offset, in axis order.
//  k_mc_faces      one lane per cell: the case's triangles; a corner on table edge e is the
//                  vertex of (cell + corner(e), axis(e)), whose index is that point's block base
//                  + local offset + popcount(mask below the axis).
//  k_cc_hook /     one union-find sweep over the faces (hook the larger roots under the
//  k_cc_compress   smallest with atomicMin), then every vertex points at its root.
//
// The neighbour signs come through L1 / L2, not an LDS tile: with the linear point index on the
// lanes each of the 8 corner loads of a wave is one coalesced row segment, 7 of them rows another
// wave has just read (DESIGN.md records the choice).
#include <cmath>

#include "geom_device.h"
#include "host_entry.h"

#pragma clang fp contract(off)

namespace nof {

// The per-point word's offsets are local to a block of MC_BLOCK points: 255 * 3 < 2^10 vertices and
// 255 * 5 < 2^11 faces precede a point in its block. k_mc_vertices / k_mc_faces find a point's block as
// p >> MC_SHIFT, whatever their own launch shape.
constexpr int MC_BLOCK = 256;
constexpr int MC_SHIFT = 8;
constexpr int MC_ROW = 16;      // bytes per case in `tables`: count, then 5 x 3 edge codes

// word = vertex offset [0,10) | crossing mask [10,13) | face offset [13,24) | case [24,32)
__device__ __forceinline__ uint32_t mc_pack(uint32_t voff, uint32_t mask, uint32_t foff, uint32_t kase) {
    return voff | (mask << 10) | (foff << 13) | (kase << 24);
}
__device__ __forceinline__ uint32_t mc_voff(uint32_t w) { return w & 0x3ffu; }
__device__ __forceinline__ uint32_t mc_mask(uint32_t w) { return (w >> 10) & 7u; }
__device__ __forceinline__ uint32_t mc_foff(uint32_t w) { return (w >> 13) & 0x7ffu; }
__device__ __forceinline__ uint32_t mc_case(uint32_t w) { return w >> 24; }

__global__ __launch_bounds__(MC_BLOCK) void k_mc_count(const float *__restrict__ vol, int n0, int n1, int n2, int P,
                                                       float level, const uint8_t *__restrict__ tables,
                                                       uint32_t *__restrict__ cells, int32_t *__restrict__ block_counts,
                                                       float *__restrict__ block_range) {
    __shared__ uint32_t s_sum[MC_BLOCK / NOF_WAVE];
    __shared__ float s_min[MC_BLOCK / NOF_WAVE], s_max[MC_BLOCK / NOF_WAVE];
    const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & (NOF_WAVE - 1), wave = threadIdx.x / NOF_WAVE;
    uint32_t mask = 0, kase = 0, nf = 0;
    float vmin = __builtin_inff(), vmax = -__builtin_inff();
    if (p < P) {
        const int k = p % n2, r = p / n2, j = r % n1, i = r / n1;
        const int s0 = n1 * n2, s1 = n2;
        const bool h0 = i + 1 < n0, h1 = j + 1 < n1, h2 = k + 1 < n2;
        const float v = vol[p];
        vmin = vmax = v;
        const uint32_t in = v < level;
        if (h0 && h1 && h2) {   // lowest corner of a cell: corner c sits at offset (c & 1, c >> 1 & 1, c >> 2 & 1)
            kase = in;
#pragma unroll
            for (int c = 1; c < 8; ++c)
                kase |= (uint32_t)(vol[p + (c & 1) * s0 + ((c >> 1) & 1) * s1 + ((c >> 2) & 1)] < level) << c;
            mask = (((kase >> 1) ^ kase) & 1u) | ((((kase >> 2) ^ kase) & 1u) << 1) | ((((kase >> 4) ^ kase) & 1u) << 2);
            nf = tables[kase * MC_ROW];
        } else {                // on an upper face of the volume: the edges that exist, no cell
            if (h0) mask |= ((uint32_t)(vol[p + s0] < level) ^ in);
            if (h1) mask |= ((uint32_t)(vol[p + s1] < level) ^ in) << 1;
            if (h2) mask |= ((uint32_t)(vol[p + 1] < level) ^ in) << 2;
        }
    }
    // vertices in the low half, faces in the high half: a block holds at most 768 and 1280
    const uint32_t cnt = (uint32_t)__popc(mask) | (nf << 16);
    uint32_t x = cnt;
#pragma unroll
    for (int d = 1; d < NOF_WAVE; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
#pragma unroll
    for (int d = NOF_WAVE / 2; d > 0; d >>= 1) {
        vmin = fminf(vmin, __shfl_xor(vmin, d));
        vmax = fmaxf(vmax, __shfl_xor(vmax, d));
    }
    if (lane == NOF_WAVE - 1) s_sum[wave] = x;
    if (lane == 0) {
        s_min[wave] = vmin;
        s_max[wave] = vmax;
    }
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; ++w) base += s_sum[w];
    const uint32_t excl = base + x - cnt;
    if (p < P) cells[p] = mc_pack(excl & 0xffffu, mask, excl >> 16, kase);
    if (threadIdx.x == MC_BLOCK - 1) {
        block_counts[2 * blockIdx.x] = (int32_t)((base + x) & 0xffffu);
        block_counts[2 * blockIdx.x + 1] = (int32_t)((base + x) >> 16);
    }
    if (threadIdx.x == 0) {
        for (int w = 1; w < MC_BLOCK / NOF_WAVE; ++w) {
            vmin = fminf(vmin, s_min[w]);
            vmax = fmaxf(vmax, s_max[w]);
        }
        block_range[2 * blockIdx.x] = vmin;
        block_range[2 * blockIdx.x + 1] = vmax;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_vertices(const float *__restrict__ vol, int n1, int n2, int P, float level,
                                                          const uint32_t *__restrict__ cells,
                                                          const int64_t *__restrict__ block_base, int64_t V,
                                                          float *__restrict__ vertices) {
    const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (p >= P) return;
    const uint32_t w = cells[p], mask = mc_mask(w);
    if (!mask) return;
    int64_t idx = block_base[2 * (p >> MC_SHIFT)] + mc_voff(w);
    const int k = p % n2, r = p / n2, j = r % n1, i = r / n1;
    const int stride[3] = {n1 * n2, n2, 1};
    const float v0 = vol[p];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!((mask >> a) & 1u)) continue;
        const float v1 = vol[p + stride[a]];
        // mesh.py: t = ((level - v0) / (v1 - v0)).clamp(0, 1); q + t * e_a (t * 1 is exact, q + 0 is q)
        const float t = fminf(fmaxf((level - v0) / (v1 - v0), 0.f), 1.f);
        if (idx < V) {
            float *o = vertices + idx * 3;
            o[0] = a == 0 ? (float)i + t : (float)i;
            o[1] = a == 1 ? (float)j + t : (float)j;
            o[2] = a == 2 ? (float)k + t : (float)k;
        }
        ++idx;
    }
}

__global__ __launch_bounds__(MC_BLOCK) void k_mc_faces(int n1, int n2, int P, const uint8_t *__restrict__ tables,
                                                       const uint32_t *__restrict__ cells,
                                                       const int64_t *__restrict__ block_base, int64_t F,
                                                       int32_t *__restrict__ faces) {
    const int p = blockIdx.x * MC_BLOCK + threadIdx.x;
    if (p >= P) return;
    const uint32_t w = cells[p];
    const uint8_t *row = tables + mc_case(w) * MC_ROW;   // case 0 on the points that own no cell: no triangle
    const int nf = row[0];
    if (!nf) return;
    int64_t f = block_base[2 * (p >> MC_SHIFT) + 1] + mc_foff(w);
    const int s0 = n1 * n2, s1 = n2;
    for (int s = 0; s < nf; ++s, ++f) {
        int32_t vi[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t code = row[1 + 3 * s + c];    // corner | axis << 3 of the table edge
            const int q = p + (int)(code & 1u) * s0 + (int)((code >> 1) & 1u) * s1 + (int)((code >> 2) & 1u);
            const uint32_t wq = cells[q];
            vi[c] = (int32_t)(block_base[2 * (q >> MC_SHIFT)] + mc_voff(wq) +
                              __popc(mc_mask(wq) & ((1u << (code >> 3)) - 1u)));
        }
        if (f < F) {
            int32_t *o = faces + f * 3;
            o[0] = vi[0];    // mesh.py flips the table's loops: corners [0, 2, 1]
            o[1] = vi[2];
            o[2] = vi[1];
        }
    }
}

__global__ __launch_bounds__(256) void k_cc_hook(const int32_t *__restrict__ faces, int64_t F, int64_t V, int32_t *labels,
                                                 int32_t *changed) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int32_t a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    if (a < 0 || b < 0 || c < 0 || a >= V || b >= V || c >= V) return;   // not a face of this mesh
    const int32_t r[3] = {uf_find(labels, a), uf_find(labels, b), uf_find(labels, c)};
    const int32_t m = min(r[0], min(r[1], r[2]));
    bool lowered = false;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (r[k] != m) lowered |= atomicMin(labels + r[k], m) > m;
    if (lowered) *changed = 1;
}

__global__ __launch_bounds__(256) void k_cc_compress(int64_t V, int32_t *labels) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    uf_compress(labels, (int32_t)v);
}

static int mc_shape(const char *fn, int32_t n0, int32_t n1, int32_t n2, int64_t *points) {
    if (n0 < 2 || n1 < 2 || n2 < 2)
        return set_error(NOF_EINVAL, "%s: volume %d x %d x %d needs at least 2 points per axis", fn, n0, n1, n2);
    const int64_t plane = (int64_t)n0 * n1;    // < 2^62; tested before the next product, which then is too
    if (plane >= (1ll << 31) || plane * n2 > ((1ll << 31) - 1) / 3)
        return set_error(NOF_EINVAL, "%s: volume %d x %d x %d: points * 3 must be below 2^31", fn, n0, n1, n2);
    *points = plane * n2;
    return 0;
}

}  // namespace nof

using namespace nof;

extern "C" {

int nof_marching_cubes_blocks(int32_t n0, int32_t n1, int32_t n2, int64_t *n_blocks) {
    int64_t P;
    if (int rc = mc_shape("marching_cubes_blocks", n0, n1, n2, &P)) return rc;
    if (!n_blocks) return set_error(NOF_EINVAL, "marching_cubes_blocks: n_blocks is NULL");
    *n_blocks = (P + MC_BLOCK - 1) / MC_BLOCK;
    return 0;
}

int nof_marching_cubes_count(const float *volume, int32_t n0, int32_t n1, int32_t n2, float level, const uint8_t *tables,
                             uint32_t *cells, int32_t *block_counts, float *block_range, void *stream) {
    const char *fn = "marching_cubes_count";
    int64_t P;
    if (int rc = mc_shape(fn, n0, n1, n2, &P)) return rc;
    if (!std::isfinite(level)) return set_error(NOF_EINVAL, "%s: level=%g must be finite", fn, (double)level);
    if (int rc = require_pointers(fn, {{volume, "volume"}, {tables, "tables"}, {cells, "cells"},
                                       {block_counts, "block_counts"}, {block_range, "block_range"}}))
        return rc;
    hipLaunchKernelGGL(k_mc_count, dim3(div_up(P, MC_BLOCK)), dim3(MC_BLOCK), 0, (hipStream_t)stream, volume, n0, n1, n2,
                       (int)P, level, tables, cells, block_counts, block_range);
    return check_launch(fn);
}

int nof_marching_cubes_emit(const float *volume, int32_t n0, int32_t n1, int32_t n2, float level, const uint8_t *tables,
                            const uint32_t *cells, const int64_t *block_base, int64_t n_vertices, int64_t n_faces,
                            float *vertices, int32_t *faces, void *stream) {
    const char *fn = "marching_cubes_emit";
    int64_t P;
    if (int rc = mc_shape(fn, n0, n1, n2, &P)) return rc;
    if (!std::isfinite(level)) return set_error(NOF_EINVAL, "%s: level=%g must be finite", fn, (double)level);
    if (n_vertices < 0 || n_vertices > 3 * P) return set_error(NOF_EINVAL, "%s: n_vertices=%lld must be in [0, 3 points]", fn, (long long)n_vertices);
    if (n_faces < 0 || n_faces > 5 * P) return set_error(NOF_EINVAL, "%s: n_faces=%lld must be in [0, 5 points]", fn, (long long)n_faces);
    if (int rc = require_pointers(fn, {{volume, "volume"}, {tables, "tables"}, {cells, "cells"}, {block_base, "block_base"},
                                       {vertices, "vertices", n_vertices > 0}, {faces, "faces", n_faces > 0}}))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    if (n_vertices > 0)
        hipLaunchKernelGGL(k_mc_vertices, dim3(div_up(P, MC_BLOCK)), dim3(MC_BLOCK), 0, s, volume, n1, n2, (int)P, level,
                           cells, block_base, n_vertices, vertices);
    if (n_faces > 0)
        hipLaunchKernelGGL(k_mc_faces, dim3(div_up(P, MC_BLOCK)), dim3(MC_BLOCK), 0, s, n1, n2, (int)P, tables, cells,
                           block_base, n_faces, faces);
    return check_launch(fn);
}

int nof_mesh_components(const int32_t *faces, int64_t n_faces, int64_t n_vertices, int32_t *labels, int32_t *changed,
                        void *stream) {
    const char *fn = "mesh_components";
    if (n_faces < 0 || n_faces * 3 >= (1ll << 31) || n_faces >= (1ll << 31))
        return set_error(NOF_EINVAL, "%s: n_faces=%lld: n_faces * 3 must be in [0, 2^31)", fn, (long long)n_faces);
    if (n_vertices < 0 || n_vertices >= (1ll << 31))
        return set_error(NOF_EINVAL, "%s: n_vertices=%lld must be in [0, 2^31)", fn, (long long)n_vertices);
    if (!changed) return set_error(NOF_EINVAL, "%s: changed is NULL", fn);
    if (n_faces > 0 && !faces) return set_error(NOF_EINVAL, "%s: faces is NULL", fn);
    if (n_vertices > 0 && !labels) return set_error(NOF_EINVAL, "%s: labels is NULL", fn);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(changed, 0, sizeof(int32_t), s) != hipSuccess)
        return set_error(NOF_ELAUNCH, "%s: memset failed", fn);
    if (n_faces == 0 || n_vertices == 0) return 0;
    hipLaunchKernelGGL(k_cc_hook, dim3(div_up(n_faces, 256)), dim3(256), 0, s, faces, n_faces, n_vertices, labels, changed);
    hipLaunchKernelGGL(k_cc_compress, dim3(div_up(n_vertices, 256)), dim3(256), 0, s, n_vertices, labels);
    return check_launch(fn);
}

}  // extern "C"
