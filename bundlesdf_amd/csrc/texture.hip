// Texture baking from the training images: the device path
// of NerfRunner.mesh_texture_from_train_images (nerf_runner.py:1467-1541).
// The reference renders each camera's depth with pyrender, back-projects it,
// snaps the points to the mesh with trimesh.proximity.closest_point, turns
// them into texel coordinates with common.rayColorToTextureImageCUDA and
// accumulates the first colour per texel with torch.unique + scatter. Here:
//
//  k_raster        one thread per face: project_face, then the lane walks the
//                  integer pixel centres of the box and splats each into the
//                  64-bit z-buffer -> depth and face id at once. raster.h holds
//                  the definition of the projection, cull, coverage, depth and
//                  key, shared with nof_render_mesh.
//  k_hits          per pixel: depth >= min_depth and the object mask ->
//                  back-projection (depth2xyzmap arithmetic), camera->object
//                  transform, closest point on the rasterised face (the
//                  reference's closest_point, restricted to the face the pixel
//                  sees) -> hit location + face id (dense, -1 = none).
//  k_tex_first /   texel = round-half-even(uv) flattened with the reference's
//  k_tex_add       row stride (W-1) (nerf_runner.py:1524-1531); the first
//                  hit (pixel order) of each texel adds its colour and weight 1.
//
// Vertex colours from the training images (SURVEY §8f row 2,
// NerfRunner.mesh_vertex_color_from_train_images, nerf_runner.py:1431-1464): the
// reference back-projects every frame's depth image, builds a cKDTree over
// the points and queries it once per vertex. Here:
//
//  k_vertex_color  one lane per vertex: the nearest back-projected pixel of
//                  the z-buffer inside the screen window that bounds every
//                  candidate within `radius` (see the kernel), its colour
//                  added to the vertex's f64 sum and 1 to its count.
#include "raster.h"
#include "host_entry.h"

#pragma clang fp contract(off)

namespace nof {

struct Cam {
    double T[12];             // rows of [R | t] (OpenCV)
    Pinhole k;
};

__global__ __launch_bounds__(256) void k_raster(const float *__restrict__ V, const int64_t *__restrict__ F,
                                                int64_t nF, Cam c, int H, int W, double znear, double zfar,
                                                unsigned long long *__restrict__ zbuf) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nF) return;
    Tri t;
    if (!project_face(V, F, f, c.T, c.k, H, W, znear, t)) return;
    for (int py = t.v0; py <= t.v1; ++py)
        for (int px = t.u0; px <= t.u1; ++px) splat(t, px, py, zfar, (uint32_t)f, W, zbuf);
}

// Pixel (px, py) of depth z in the object frame: depth2xyzmap (Utils.py:219-231, f64 arithmetic,
// f32 result) followed by cam_in_ob (`inv`) in f64.
__device__ __forceinline__ void backproject(const Cam &inv, int px, int py, float z, double p[3]) {
    const float xc = (float)(((double)px - inv.k.cx) * (double)z / inv.k.fx);
    const float yc = (float)(((double)py - inv.k.cy) * (double)z / inv.k.fy);
    xform_point(inv.T, (double)xc, (double)yc, (double)z, p);
}

// Closest point of triangle (a, b, c) to p (Voronoi-region walk, f64).
__device__ __forceinline__ void closest_on_tri(const double p[3], const double a[3], const double b[3],
                                               const double c[3], double out[3]) {
    double ab[3], ac[3], ap[3];
    for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = p[k] - a[k]; }
    auto dot = [](const double *x, const double *y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; };
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0 && d2 <= 0) { for (int k = 0; k < 3; ++k) out[k] = a[k]; return; }
    double bp[3];
    for (int k = 0; k < 3; ++k) bp[k] = p[k] - b[k];
    const double d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0 && d4 <= d3) { for (int k = 0; k < 3; ++k) out[k] = b[k]; return; }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0 && d1 >= 0 && d3 <= 0) {
        const double t = d1 / (d1 - d3);
        for (int k = 0; k < 3; ++k) out[k] = a[k] + t * ab[k];
        return;
    }
    double cp[3];
    for (int k = 0; k < 3; ++k) cp[k] = p[k] - c[k];
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0 && d5 <= d6) { for (int k = 0; k < 3; ++k) out[k] = c[k]; return; }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0 && d2 >= 0 && d6 <= 0) {
        const double t = d2 / (d2 - d6);
        for (int k = 0; k < 3; ++k) out[k] = a[k] + t * ac[k];
        return;
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) {
        const double t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        for (int k = 0; k < 3; ++k) out[k] = b[k] + t * (c[k] - b[k]);
        return;
    }
    const double den = 1.0 / ((va + vb) + vc);
    const double s = vb * den, t = vc * den;
    for (int k = 0; k < 3; ++k) out[k] = (a[k] + ab[k] * s) + ac[k] * t;
}

__global__ __launch_bounds__(256) void k_hits(const unsigned long long *__restrict__ zbuf, int H, int W,
                                              const uint8_t *__restrict__ mask, float min_depth,
                                              const float *__restrict__ V, const int64_t *__restrict__ F,
                                              Cam inv, float *__restrict__ loc, int64_t *__restrict__ face) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * W) return;
    const unsigned long long key = zbuf[i];
    face[i] = -1;
    if (key == ~0ull || !mask[i]) return;
    const float z = __uint_as_float((uint32_t)(key >> 32));
    if (!(z >= min_depth)) return;
    const int64_t f = (int64_t)(key & 0xffffffffull);
    const int py = i / W, px = i - py * W;
    double p[3];
    backproject(inv, px, py, z, p);
    double a[3], b[3], c[3], q[3];
    for (int k = 0; k < 3; ++k) {
        a[k] = V[F[f * 3] * 3 + k];
        b[k] = V[F[f * 3 + 1] * 3 + k];
        c[k] = V[F[f * 3 + 2] * 3 + k];
    }
    closest_on_tri(p, a, b, c, q);
    for (int k = 0; k < 3; ++k) loc[(size_t)i * 3 + k] = (float)q[k];
    face[i] = f;
}

// Pixel range [lo, hi] that x / z * f + c can reach for x in [x0, x1], z in [z0, z1], z0 > 0: the
// expression is monotone in x and in z, so its extremes are at the four corners. Floor / ceil,
// one more pixel each way, clamped to [0, n - 1]; false where nothing is left (or a NaN came in).
__device__ __forceinline__ bool pixel_range(double f, double c, double x0, double x1, double z0, double z1, int n,
                                            int &lo, int &hi) {
    const double a = f * x0 / z0 + c, b = f * x0 / z1 + c, d = f * x1 / z0 + c, e = f * x1 / z1 + c;
    const double l = fmax(floor(fmin(fmin(a, b), fmin(d, e))) - 1.0, 0.0);
    const double h = fmin(ceil(fmax(fmax(a, b), fmax(d, e))) + 1.0, (double)(n - 1));
    if (!(l <= h)) return false;
    lo = (int)l;
    hi = (int)h;
    return true;
}

// One lane per vertex. The candidates are k_hits' pixels (a face, the mask, z >= min_depth) and a
// candidate's point is k_hits' p (backproject). The match is the candidate with the smallest
// d2 = (dx*dx + dy*dy) + dz*dz, ties to the lowest pixel index (the window is walked in pixel
// order and only a strictly smaller d2 replaces the best), accepted where sqrt(d2) <= radius.
//
// Search window. In the camera frame the vertex is (Xv, Yv, Zv) and a candidate is
// (xc, yc, z) with xc = (px - cx) * z / fx, so px = fx * xc / z + cx. cam_in_ob is rigid, so a
// candidate within r = radius of the vertex has |xc - Xv| <= r, |yc - Yv| <= r, |z - Zv| <= r, and
// z >= min_depth > 0 besides. fx * x / z + cx is monotone in x and in z for z > 0, hence px lies
// between the min and the max of that expression over the corners of [Xv - r, Xv + r] x
// [max(Zv - r, min_depth), Zv + r], and py likewise. The range is floored / ceiled and widened
// by one pixel: the f32 rounding of xc and yc moves px by 2^-24 |px - cx|, and ob_in_cam being
// only the computed inverse of cam_in_ob (or a rotation orthonormal only to f32) moves it by
// about 1e-7 of the window, both far below a pixel. Zv + r < min_depth or a range that misses the
// image means there is no candidate within r, and pixels of the window that lie beyond r are
// rejected by the distance test itself: what is reported never depends on the window.
//
// One vertex is one lane's, so the sums are plain read-modify-writes: no atomics, and the
// result does not depend on the launch shape.
__global__ __launch_bounds__(256) void k_vertex_color(const unsigned long long *__restrict__ zbuf, int H, int W,
                                                      const uint8_t *__restrict__ mask, float min_depth,
                                                      const float *__restrict__ colors, Cam inv, Cam c,
                                                      const float *__restrict__ V, int64_t nV, double radius,
                                                      double *__restrict__ color_sum, int32_t *__restrict__ count,
                                                      int32_t *__restrict__ nearest,
                                                      double *__restrict__ nearest_dist) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nV) return;
    const double vx = V[j * 3], vy = V[j * 3 + 1], vz = V[j * 3 + 2];
    double Xc[3];
    xform_point(c.T, vx, vy, vz, Xc);
    const double Xv = Xc[0], Yv = Xc[1], Zv = Xc[2];
    const double z0 = fmax(Zv - radius, (double)min_depth), z1 = Zv + radius;
    double best = __builtin_inf();
    int best_i = -1;
    int u0, u1, v0, v1;
    if (z0 <= z1 && pixel_range(c.k.fx, c.k.cx, Xv - radius, Xv + radius, z0, z1, W, u0, u1) &&
        pixel_range(c.k.fy, c.k.cy, Yv - radius, Yv + radius, z0, z1, H, v0, v1)) {
        for (int py = v0; py <= v1; ++py)
            for (int px = u0; px <= u1; ++px) {
                const int i = py * W + px;
                const unsigned long long key = zbuf[i];
                if (key == ~0ull || !mask[i]) continue;
                const float z = __uint_as_float((uint32_t)(key >> 32));
                if (!(z >= min_depth)) continue;
                double p[3];
                backproject(inv, px, py, z, p);
                const double dx = p[0] - vx, dy = p[1] - vy, dz = p[2] - vz;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < best) {
                    best = d2;
                    best_i = i;
                }
            }
    }
    const double dist = sqrt(best);
    const bool ok = best_i >= 0 && dist <= radius;
    if (ok) {
        const float *col = colors + (size_t)best_i * 3;
        double *s = color_sum + j * 3;
        s[0] += (double)col[0];
        s[1] += (double)col[1];
        s[2] += (double)col[2];
        count[j] += 1;
    }
    if (nearest) nearest[j] = ok ? best_i : -1;
    if (nearest_dist) nearest_dist[j] = ok ? dist : __builtin_inf();
}

__device__ __forceinline__ int64_t texel_flat(const float *uv, int TW) {
    const int64_t x = (int64_t)rint(uv[0]), y = (int64_t)rint(uv[1]);   // torch.round: half to even
    return y * (TW - 1) + x;
}

__global__ __launch_bounds__(256) void k_tex_first(const float *__restrict__ uvs, int64_t M, int TW,
                                                   int64_t n_first, int32_t *__restrict__ first) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= M) return;
    const int64_t fl = texel_flat(uvs + k * 2, TW);
    if (fl >= 0 && fl < n_first) atomicMin(&first[fl], (int32_t)k);
}

__global__ __launch_bounds__(256) void k_tex_add(const float *__restrict__ uvs, const int32_t *__restrict__ pix,
                                                 int64_t M, const float *__restrict__ img, int TH, int TW,
                                                 int64_t n_first, int32_t *__restrict__ first,
                                                 float *__restrict__ tex, float *__restrict__ wtex) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= M) return;
    const int64_t fl = texel_flat(uvs + k * 2, TW);
    if (fl < 0 || fl >= n_first || first[fl] != (int32_t)k) return;
    first[fl] = 0x7fffffff;                 // reset for the next frame (only the winner writes)
    const int64_t ux = fl % (TW - 1), uy = fl / (TW - 1);
    if (uy >= TH) return;                   // (W-1)-stride alias of the last texel: outside the image
    const float *col = img + (size_t)pix[k] * 3;
    float *t = tex + ((size_t)uy * TW + ux) * 3;
    t[0] += col[0];
    t[1] += col[1];
    t[2] += col[2];
    wtex[(size_t)uy * TW + ux] += 1.f;
}

static Cam make_cam(const double *T, const double *K) {
    Cam c;
    for (int k = 0; k < 12; ++k) c.T[k] = T[k];
    c.k = {K[0], K[4], K[2], K[5]};
    return c;
}

}  // namespace nof

using namespace nof;

extern "C" {

int nof_raster_faces(const float *V, const int64_t *F, int64_t n_faces, const double *ob_in_cam, const double *K,
                     int32_t H, int32_t W, double znear, double zfar, uint64_t *zbuf, void *stream) {
    if (n_faces < 0 || H <= 0 || W <= 0 || !ob_in_cam || !K || !zbuf || (n_faces > 0 && (!V || !F)))
        return set_error(NOF_EINVAL, "raster_faces: bad arguments");
    if (n_faces >= (1ll << 32)) return set_error(NOF_EINVAL, "raster_faces: more than 2^32 faces");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(zbuf, 0xff, (size_t)H * W * 8, s) != hipSuccess)
        return set_error(NOF_ELAUNCH, "raster_faces: memset failed");
    if (n_faces == 0) return 0;
    hipLaunchKernelGGL(k_raster, dim3(div_up(n_faces, 256)), dim3(256), 0, s, V, F, n_faces, make_cam(ob_in_cam, K),
                       H, W, znear, zfar, (unsigned long long *)zbuf);
    return check_launch("raster_faces");
}

int nof_texture_hits(const uint64_t *zbuf, int32_t H, int32_t W, const uint8_t *mask, float min_depth, const float *V,
                     const int64_t *F, const double *cam_in_ob, const double *K, float *hit_locations,
                     int64_t *hit_face_ids, void *stream) {
    if (H <= 0 || W <= 0 || !zbuf || !mask || !V || !F || !cam_in_ob || !K || !hit_locations || !hit_face_ids)
        return set_error(NOF_EINVAL, "texture_hits: bad arguments");
    hipLaunchKernelGGL(k_hits, dim3(div_up((uint64_t)H * W, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned long long *)zbuf, H, W, mask, min_depth, V, F, make_cam(cam_in_ob, K),
                       hit_locations, hit_face_ids);
    return check_launch("texture_hits");
}

int nof_texture_accumulate(const float *uvs, const int32_t *pix, int64_t n_hits, const float *colors, int32_t tex_h,
                           int32_t tex_w, int32_t *first, float *tex, float *weight, void *stream) {
    if (n_hits < 0 || tex_h <= 0 || tex_w <= 1 || !first || !tex || !weight || (n_hits > 0 && (!uvs || !pix || !colors)))
        return set_error(NOF_EINVAL, "texture_accumulate: bad arguments");
    if (n_hits >= (1ll << 31)) return set_error(NOF_EINVAL, "texture_accumulate: too many hits");
    if (n_hits == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_first = (int64_t)tex_h * (tex_w - 1) + tex_w;
    hipLaunchKernelGGL(k_tex_first, dim3(div_up(n_hits, 256)), dim3(256), 0, s, uvs, n_hits, tex_w, n_first, first);
    hipLaunchKernelGGL(k_tex_add, dim3(div_up(n_hits, 256)), dim3(256), 0, s, uvs, pix, n_hits, colors, tex_h, tex_w,
                       n_first, first, tex, weight);
    return check_launch("texture_accumulate");
}

int nof_vertex_color_accumulate(const uint64_t *zbuf, int32_t H, int32_t W, const uint8_t *mask, float min_depth,
                                const float *colors, const double *cam_in_ob, const double *ob_in_cam, const double *K,
                                const float *V, int64_t n_vertices, double radius, double *color_sum, int32_t *count,
                                int32_t *nearest, double *nearest_dist, void *stream) {
    const char *fn = "vertex_color_accumulate";
    if (H <= 0 || W <= 0) return set_error(NOF_EINVAL, "%s: H=%d, W=%d must be positive", fn, H, W);
    if ((int64_t)H * W >= (1ll << 31)) return set_error(NOF_EINVAL, "%s: H*W=%lld must be below 2^31", fn, (long long)H * W);
    if (n_vertices < 0 || n_vertices >= (1ll << 31))
        return set_error(NOF_EINVAL, "%s: n_vertices=%lld must be in [0, 2^31)", fn, (long long)n_vertices);
    if (!std::isfinite(radius) || radius <= 0) return set_error(NOF_EINVAL, "%s: radius=%g must be finite and > 0", fn, radius);
    if (!(min_depth > 0)) return set_error(NOF_EINVAL, "%s: min_depth=%g must be > 0", fn, (double)min_depth);
    if (int rc = require_pointers(fn, {{zbuf, "zbuf"}, {mask, "mask"}, {colors, "colors"}, {cam_in_ob, "cam_in_ob"},
                                       {ob_in_cam, "ob_in_cam"}, {K, "K"}, {V, "V", n_vertices > 0},
                                       {color_sum, "color_sum", n_vertices > 0}, {count, "count", n_vertices > 0}}))
        return rc;
    if (n_vertices == 0) return 0;
    hipLaunchKernelGGL(k_vertex_color, dim3(div_up(n_vertices, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned long long *)zbuf, H, W, mask, min_depth, colors, make_cam(cam_in_ob, K),
                       make_cam(ob_in_cam, K), V, n_vertices, radius, color_sum, count, nearest, nearest_dist);
    return check_launch(fn);
}

}  // extern "C"
