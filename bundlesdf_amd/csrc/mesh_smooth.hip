// Mesh smoothing on the device: the explicit Laplacian / Taubin step with the
// volume constraint, and geometric vertex normals — the tail of the reference's
// postprocess_mesh (run_custom.py:158-188, trimesh.smoothing.filter_laplacian
// there). Everything is float64 in a stated operation order, without
// contraction and without floating-point atomics: two runs give the same bits.
//
//  k_laplacian_step   one thread per vertex, a Jacobi step from v_in to v_out:
//                     w = 1 / d, m = ((w v[j0] + w v[j1]) + ...) over the CSR row
//                     in stored order, out = v + factor (m - v). d == 0: copied.
//  k_mesh_volume      grid-stride over the faces, term = (x0 cx + y0 cy) + z0 cz
//                     with c = v1 x v2; butterfly over the wave, the four waves
//                     added in order, one partial per block. k_mesh_volume_final
//                     adds the partials in block order and divides by 6.
//  k_scale_to_volume  one thread per coordinate: s = cbrt(target / now), both
//                     read from device memory; a ratio that is not positive and
//                     finite leaves the vertices alone and sets *flag.
//  k_vertex_normals   one thread per vertex: the unnormalised (v1 - v0) x (v2 - v0)
//                     of its faces (vertex -> face CSR, ascending face index) added
//                     in that order, then divided by the sum's length.
#include "geom_device.h"

#pragma clang fp contract(off)

namespace nof {

constexpr int VOLUME_BLOCKS = 1024;

__global__ __launch_bounds__(256) void k_laplacian_step(const double *__restrict__ v_in,
                                                        const int32_t *__restrict__ row_start,
                                                        const int32_t *__restrict__ cols, int64_t V, double factor,
                                                        double *__restrict__ v_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const double x = v_in[i * 3], y = v_in[i * 3 + 1], z = v_in[i * 3 + 2];
    const int32_t s = row_start[i], e = row_start[i + 1];
    double ox = x, oy = y, oz = z;
    if (e > s) {
        const double w = 1.0 / (double)(e - s);
        double mx = 0.0, my = 0.0, mz = 0.0;
        for (int32_t k = s; k < e; ++k) {
            const int64_t j = cols[k];
            const bool in = j >= 0 && j < V;    // a column outside [0, V) stands for the vertex itself
            const double px = in ? v_in[j * 3] : x, py = in ? v_in[j * 3 + 1] : y, pz = in ? v_in[j * 3 + 2] : z;
            if (k == s) {
                mx = w * px;
                my = w * py;
                mz = w * pz;
            } else {
                mx = mx + w * px;
                my = my + w * py;
                mz = mz + w * pz;
            }
        }
        ox = x + factor * (mx - x);
        oy = y + factor * (my - y);
        oz = z + factor * (mz - z);
    }
    v_out[i * 3] = ox;
    v_out[i * 3 + 1] = oy;
    v_out[i * 3 + 2] = oz;
}

__global__ __launch_bounds__(256) void k_mesh_volume(const double *__restrict__ v, const int32_t *__restrict__ faces,
                                                     int64_t F, double *__restrict__ partial) {
    __shared__ double wave_sum[4][1];
    double acc[1] = {0.0};
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < F; f += stride) {
        const int64_t a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
        const double x0 = v[a * 3], y0 = v[a * 3 + 1], z0 = v[a * 3 + 2];
        const double x1 = v[b * 3], y1 = v[b * 3 + 1], z1 = v[b * 3 + 2];
        const double x2 = v[c * 3], y2 = v[c * 3 + 1], z2 = v[c * 3 + 2];
        const double cx = y1 * z2 - z1 * y2, cy = z1 * x2 - x1 * z2, cz = x1 * y2 - y1 * x2;
        acc[0] += (x0 * cx + y0 * cy) + z0 * cz;
    }
    block_sum<1>(acc, wave_sum, partial + blockIdx.x);
}

__global__ __launch_bounds__(64) void k_mesh_volume_final(const double *__restrict__ partial, int32_t n_blocks,
                                                          double *__restrict__ out) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int32_t b = 0; b < n_blocks; ++b) s += partial[b];
    *out = s / 6.0;
}

__global__ __launch_bounds__(256) void k_scale_to_volume(double *__restrict__ v, int64_t n,
                                                         const double *__restrict__ vol_target,
                                                         const double *__restrict__ vol_now,
                                                         int32_t *__restrict__ flag) {
    const double r = *vol_target / *vol_now;
    if (!(r > 0.0 && r < __longlong_as_double(0x7ff0000000000000ll))) {   // NaN fails both
        if (blockIdx.x == 0 && threadIdx.x == 0) *flag = 1;
        return;
    }
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = v[i] * cbrt(r);
}

__global__ __launch_bounds__(256) void k_vertex_normals(const double *__restrict__ v, const int32_t *__restrict__ faces,
                                                        const int32_t *__restrict__ face_row_start,
                                                        const int32_t *__restrict__ face_ids, int64_t V,
                                                        double *__restrict__ normals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    const int32_t e = face_row_start[i + 1];
    for (int32_t k = face_row_start[i]; k < e; ++k) {
        const int64_t f = face_ids[k];
        const int64_t a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
        if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) continue;   // no out-of-range read
        const double x0 = v[a * 3], y0 = v[a * 3 + 1], z0 = v[a * 3 + 2];
        const double ux = v[b * 3] - x0, uy = v[b * 3 + 1] - y0, uz = v[b * 3 + 2] - z0;
        const double wx = v[c * 3] - x0, wy = v[c * 3 + 1] - y0, wz = v[c * 3 + 2] - z0;
        sx = sx + (uy * wz - uz * wy);
        sy = sy + (uz * wx - ux * wz);
        sz = sz + (ux * wy - uy * wx);
    }
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    const bool ok = len > 0.0;      // a zero (or NaN) sum gives (0, 0, 0)
    normals[i * 3] = ok ? sx / len : 0.0;
    normals[i * 3 + 1] = ok ? sy / len : 0.0;
    normals[i * 3 + 2] = ok ? sz / len : 0.0;
}

static int32_t volume_blocks(int64_t F) {
    const int64_t nb = (F + 255) / 256;
    return (int32_t)(nb < 1 ? 1 : (nb < VOLUME_BLOCKS ? nb : VOLUME_BLOCKS));
}

static int bad_count(const char *fn, const char *name, int64_t n) {
    return set_error(NOF_EINVAL, "%s: %s=%lld: %s * 3 must be in [0, 2^31)", fn, name, (long long)n, name);
}

static bool count_ok(int64_t n) { return n >= 0 && n * 3 < (1ll << 31); }

}  // namespace nof

using namespace nof;

extern "C" {

int nof_mesh_laplacian_step(const double *v_in, const int32_t *row_start, const int32_t *cols, int64_t V, double factor,
                            double *v_out, void *stream) {
    const char *fn = "mesh_laplacian_step";
    if (!count_ok(V)) return bad_count(fn, "V", V);
    if (!(factor - factor == 0.0)) return set_error(NOF_EINVAL, "%s: factor must be finite", fn);
    if (V == 0) return 0;
    if (!v_in || !v_out || !row_start) return set_error(NOF_EINVAL, "%s: NULL input/output pointer", fn);
    if (v_in == v_out) return set_error(NOF_EINVAL, "%s: v_in and v_out must be distinct buffers (a Jacobi step)", fn);
    hipLaunchKernelGGL(k_laplacian_step, dim3(div_up(V, 256)), dim3(256), 0, (hipStream_t)stream, v_in, row_start, cols,
                       V, factor, v_out);
    return check_launch(fn);
}

size_t nof_mesh_volume_workspace_bytes(int64_t F) { return (size_t)volume_blocks(F) * sizeof(double); }

int nof_mesh_volume(const double *vertices, const int32_t *faces, int64_t F, double *volume_out, void *workspace,
                    void *stream) {
    const char *fn = "mesh_volume";
    if (!count_ok(F)) return bad_count(fn, "F", F);
    if (!volume_out || !workspace) return set_error(NOF_EINVAL, "%s: volume_out / workspace is NULL", fn);
    if (F > 0 && (!vertices || !faces)) return set_error(NOF_EINVAL, "%s: NULL vertices / faces", fn);
    const int32_t nb = F > 0 ? volume_blocks(F) : 0;
    if (nb > 0)
        hipLaunchKernelGGL(k_mesh_volume, dim3(nb), dim3(256), 0, (hipStream_t)stream, vertices, faces, F,
                           (double *)workspace);
    hipLaunchKernelGGL(k_mesh_volume_final, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double *)workspace, nb,
                       volume_out);
    return check_launch(fn);
}

int nof_mesh_scale_to_volume(double *vertices, int64_t V, const double *vol_target, const double *vol_now, int32_t *flag,
                             void *stream) {
    const char *fn = "mesh_scale_to_volume";
    if (!count_ok(V)) return bad_count(fn, "V", V);
    if (!vol_target || !vol_now || !flag) return set_error(NOF_EINVAL, "%s: vol_target / vol_now / flag is NULL", fn);
    if (V > 0 && !vertices) return set_error(NOF_EINVAL, "%s: vertices is NULL", fn);
    const uint32_t nb = V > 0 ? div_up(V * 3, 256) : 1;     // V == 0 still reports a bad ratio
    hipLaunchKernelGGL(k_scale_to_volume, dim3(nb), dim3(256), 0, (hipStream_t)stream, vertices, V * 3, vol_target,
                       vol_now, flag);
    return check_launch(fn);
}

int nof_mesh_vertex_normals(const double *vertices, const int32_t *faces, const int32_t *face_row_start,
                            const int32_t *face_ids, int64_t V, double *normals_out, void *stream) {
    const char *fn = "mesh_vertex_normals";
    if (!count_ok(V)) return bad_count(fn, "V", V);
    if (V == 0) return 0;
    if (!vertices || !face_row_start || !normals_out) return set_error(NOF_EINVAL, "%s: NULL input/output pointer", fn);
    hipLaunchKernelGGL(k_vertex_normals, dim3(div_up(V, 256)), dim3(256), 0, (hipStream_t)stream, vertices, faces,
                       face_row_start, face_ids, V, normals_out);
    return check_launch(fn);
}

}  // extern "C"
