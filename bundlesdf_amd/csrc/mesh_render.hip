// Mesh render (nof_render_mesh): depth, face id, colour and normal images of a triangle mesh at B
// poses, the device counterpart of the reference's pyrender pass (offscreen_renderer.py:
// ModelRendererOffscreen). Three kernels on one stream, nothing read back:
//
//  k_mesh_setup   one lane per (pose, face): project_face (raster.h holds the definition of the
//                 projection, cull, coverage, depth and key, shared with nof_raster_faces). A box of
//                 at most small_max_pixels pixels is walked by the lane itself (splat into the pose's
//                 z-buffer). Any other face is appended to the list of large faces: one counter
//                 increment per wave (ballot, prefix count, one atomicAdd by the first listing lane).
//                 The list has a slot for every (pose, face).
//  k_mesh_large   one wave per list entry, a fixed grid striding over the list (the count is read
//                 from device memory). The 64 lanes take consecutive pixels of the bounding box in
//                 row-major order, so a wave's atomics land on neighbouring addresses and a
//                 screen-filling triangle costs its pixels / 64 per lane. Same cover, same keys.
//  k_mesh_shade   one lane per (pose, pixel). A miss (key all ones) writes depth 0, face -1, rgb 0,
//                 normal 0. A hit, for face f = low 32 bits of the key at pixel (px, py):
//                   1. project_face and cover as above: e0, e1, e2, zi (the same bits as in the
//                      raster step); depth = the key's high 32 bits (= (float)zi), face = f.
//                   2. w_k = (e_k / z_k) * zi, f64.
//                   3. n = (w0 n_0 + w1 n_1) + w2 n_2 per component with vertex normals (f32 widened
//                      to f64), else the face normal a x b, a = p1 - p0, b = p2 - p0 (object frame,
//                      f64): (a_y b_z - a_z b_y, a_z b_x - a_x b_z, a_x b_y - a_y b_x).
//                   4. camera frame: m = xform_dir(T, n), the rotation alone; l = sqrt((m_x m_x +
//                      m_y m_y) + m_z m_z); l > 0: m = m / l (a zero normal stays zero).
//                   5. pixel ray d = ((px - cx) / fx, (py - cy) / fy, 1) / sqrt((d_x d_x + d_y d_y) + 1);
//                      c = (m_x d_x + m_y d_y) + m_z d_z; c > 0: m = -m. normal = (float)m.
//                   6. colour per channel, f64. vertex: (w0 c_0 + w1 c_1) + w2 c_2 of the u8 colours.
//                      texture: s = (w0 s_0 + w1 s_1) + w2 s_2 for both uv components, column
//                      rint(s_u (TW - 1)), row (TH - 1) - rint(s_v (TH - 1)), both clamped into the
//                      image (a NaN reads column / row 0 before the flip), the texel's u8 colour.
//                      flat: base_rgb.
//                   7. shade: colour = colour * |c|.
//                   8. rgb = rint(colour) (half to even) clamped to 0 .. 255.
//
// All of it is IEEE f64 + - * / sqrt in the stated order with contraction off; tests/mesh_render_oracle.py
// restates steps 2-8 in numpy and the z-buffer is oracle/texture.py's raster.
#include "raster.h"
#include "host_entry.h"

#pragma clang fp contract(off)

namespace nof {

__global__ __launch_bounds__(256) void k_mesh_setup(const float *__restrict__ V, const int64_t *__restrict__ F,
                                                    int64_t nF, const double *__restrict__ poses, int64_t n_items,
                                                    Pinhole c, int H, int W, double znear, double zfar,
                                                    int small_max, unsigned long long *__restrict__ zbuf,
                                                    unsigned long long *__restrict__ list,
                                                    unsigned int *__restrict__ n_large) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t b = 0, f = 0;
    Tri t;
    bool live = i < n_items;
    if (live) {
        b = i / nF;
        f = i - b * nF;
        live = project_face(V, F, f, poses + b * 16, c, H, W, znear, t);
    }
    const int64_t pixels = live ? (int64_t)(t.u1 - t.u0 + 1) * (int64_t)(t.v1 - t.v0 + 1) : 0;   // both factors >= 1
    const bool large = live && pixels > (int64_t)small_max;
    // the append: one counter increment per wave
    const unsigned long long m = __ballot(large);
    if (m != 0ull) {
        const int lane = threadIdx.x & 63;
        const int leader = __ffsll((long long)m) - 1;
        unsigned int base = 0;
        if (lane == leader) base = atomicAdd(n_large, (unsigned int)__popcll(m));
        base = __shfl(base, leader, 64);
        if (large) list[base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull))] = ((unsigned long long)b << 32) | (unsigned long long)f;
    }
    if (!live || large) return;
    unsigned long long *zb = zbuf + (size_t)b * H * W;
    for (int py = t.v0; py <= t.v1; ++py)
        for (int px = t.u0; px <= t.u1; ++px) splat(t, px, py, zfar, (uint32_t)f, W, zb);
}

__global__ __launch_bounds__(256) void k_mesh_large(const float *__restrict__ V, const int64_t *__restrict__ F,
                                                    const double *__restrict__ poses, Pinhole c, int H, int W,
                                                    double znear, double zfar, unsigned long long *__restrict__ zbuf,
                                                    const unsigned long long *__restrict__ list,
                                                    const unsigned int *__restrict__ n_large) {
    const unsigned int n = *n_large;
    const unsigned int waves = gridDim.x * 4u;
    const int lane = threadIdx.x & 63;
    for (unsigned int i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += waves) {
        const unsigned long long entry = list[i];
        const int64_t b = (int64_t)(entry >> 32), f = (int64_t)(entry & 0xffffffffull);
        Tri t;
        if (!project_face(V, F, f, poses + b * 16, c, H, W, znear, t)) continue;   // listed faces passed it already
        const int bw = t.u1 - t.u0 + 1;
        const int64_t pixels = (int64_t)bw * (int64_t)(t.v1 - t.v0 + 1);
        unsigned long long *zb = zbuf + (size_t)b * H * W;
        for (int64_t p = lane; p < pixels; p += 64) {
            const int row = (int)(p / bw);
            splat(t, t.u0 + (int)(p - (int64_t)row * bw), t.v0 + row, zfar, (uint32_t)f, W, zb);
        }
    }
}

struct MeshShade {
    const uint8_t *colors;
    const float *normals;
    const float *uv;
    const uint8_t *texture;
    int tex_h, tex_w, mode, shade;
    double base[3];
};

__device__ __forceinline__ double mix3(const double w[3], double a, double b, double c) {
    return (w[0] * a + w[1] * b) + w[2] * c;
}

__global__ __launch_bounds__(256) void k_mesh_shade(const float *__restrict__ V, const int64_t *__restrict__ F,
                                                    const double *__restrict__ poses, int64_t n_pixels, Pinhole c,
                                                    int H, int W, double znear, double zfar, MeshShade s,
                                                    const unsigned long long *__restrict__ zbuf,
                                                    float *__restrict__ depth, int32_t *__restrict__ face,
                                                    uint8_t *__restrict__ rgb, float *__restrict__ normal) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pixels) return;
    const unsigned long long key = zbuf[i];
    float od = 0.f, on[3] = {0.f, 0.f, 0.f};
    int32_t of = -1;
    uint8_t oc[3] = {0, 0, 0};
    const int64_t b = i / ((int64_t)H * W);
    const int p = (int)(i - b * (int64_t)H * W);
    const int py = p / W, px = p - py * W;
    const double *T = poses + b * 16;
    const int64_t f = (int64_t)(key & 0xffffffffull);
    Tri t;
    double e[3], zi;
    // a key can only have come from a face that projects and covers this pixel: the test cannot fail
    if (key != ~0ull && project_face(V, F, f, T, c, H, W, znear, t) && cover(t, px, py, zfar, e, zi)) {
        od = __uint_as_float((uint32_t)(key >> 32));
        of = (int32_t)f;
        const double w[3] = {(e[0] / t.z[0]) * zi, (e[1] / t.z[1]) * zi, (e[2] / t.z[2]) * zi};
        const int64_t i0 = F[f * 3], i1 = F[f * 3 + 1], i2 = F[f * 3 + 2];
        double n[3];
        if (s.normals) {
            for (int k = 0; k < 3; ++k)
                n[k] = mix3(w, (double)s.normals[i0 * 3 + k], (double)s.normals[i1 * 3 + k], (double)s.normals[i2 * 3 + k]);
        } else {
            double a[3], d[3];
            for (int k = 0; k < 3; ++k) {
                a[k] = (double)V[i1 * 3 + k] - (double)V[i0 * 3 + k];
                d[k] = (double)V[i2 * 3 + k] - (double)V[i0 * 3 + k];
            }
            n[0] = a[1] * d[2] - a[2] * d[1];
            n[1] = a[2] * d[0] - a[0] * d[2];
            n[2] = a[0] * d[1] - a[1] * d[0];
        }
        double m[3];
        xform_dir(T, n[0], n[1], n[2], m);
        const double l = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
        if (l > 0.0) {
            m[0] = m[0] / l;
            m[1] = m[1] / l;
            m[2] = m[2] / l;
        }
        double d[3] = {((double)px - c.cx) / c.fx, ((double)py - c.cy) / c.fy, 1.0};
        const double dl = sqrt((d[0] * d[0] + d[1] * d[1]) + 1.0);
        d[0] = d[0] / dl;
        d[1] = d[1] / dl;
        d[2] = d[2] / dl;
        const double cs = (m[0] * d[0] + m[1] * d[1]) + m[2] * d[2];
        if (cs > 0.0) {
            m[0] = -m[0];
            m[1] = -m[1];
            m[2] = -m[2];
        }
        for (int k = 0; k < 3; ++k) on[k] = (float)m[k];
        double col[3];
        if (s.mode == NOF_MESH_COLOUR_VERTEX) {
            for (int k = 0; k < 3; ++k)
                col[k] = mix3(w, (double)s.colors[i0 * 3 + k], (double)s.colors[i1 * 3 + k], (double)s.colors[i2 * 3 + k]);
        } else if (s.mode == NOF_MESH_COLOUR_TEXTURE) {
            const double su = mix3(w, (double)s.uv[i0 * 2], (double)s.uv[i1 * 2], (double)s.uv[i2 * 2]);
            const double sv = mix3(w, (double)s.uv[i0 * 2 + 1], (double)s.uv[i1 * 2 + 1], (double)s.uv[i2 * 2 + 1]);
            const double cw = (double)(s.tex_w - 1), ch = (double)(s.tex_h - 1);
            const int tc = (int)fmin(fmax(rint(su * cw), 0.0), cw);
            const int tr = s.tex_h - 1 - (int)fmin(fmax(rint(sv * ch), 0.0), ch);
            const uint8_t *tx = s.texture + ((size_t)tr * s.tex_w + tc) * 3;
            for (int k = 0; k < 3; ++k) col[k] = (double)tx[k];
        } else {
            for (int k = 0; k < 3; ++k) col[k] = s.base[k];
        }
        if (s.shade) {
            const double a = fabs(cs);
            for (int k = 0; k < 3; ++k) col[k] = col[k] * a;
        }
        for (int k = 0; k < 3; ++k) oc[k] = (uint8_t)fmin(fmax(rint(col[k]), 0.0), 255.0);
    }
    depth[i] = od;
    face[i] = of;
    for (int k = 0; k < 3; ++k) {
        rgb[i * 3 + k] = oc[k];
        normal[i * 3 + k] = on[k];
    }
}

// workspace: [0, 256) the large-face counter, then the z-buffers [B,H,W] u64, then the list [B n_faces] u64
static const size_t kMeshHead = 256;

}  // namespace nof

using namespace nof;

extern "C" {

size_t nof_render_mesh_workspace_bytes(int32_t B, int64_t n_faces, int32_t H, int32_t W) {
    if (B < 1 || H < 1 || W < 1 || n_faces < 0) return 0;
    return kMeshHead + ((size_t)B * H * W + (size_t)B * (size_t)n_faces) * 8;
}

int nof_render_mesh(const nof_mesh_render_desc *d, void *stream) {
    const char *fn = "render_mesh";
    if (!d) return set_error(NOF_EINVAL, "%s: desc is NULL", fn);
    if (d->B < 1 || d->H < 1 || d->W < 1)
        return set_error(NOF_EINVAL, "%s: B=%d, H=%d, W=%d must be positive", fn, d->B, d->H, d->W);
    if ((int64_t)d->B * d->H * d->W >= (1ll << 31))
        return set_error(NOF_EINVAL, "%s: B*H*W=%lld must be below 2^31", fn, (long long)d->B * d->H * d->W);
    // the large-face counter and the list's indices are 32 bits wide
    if (d->n_faces < 0 || d->n_faces >= (1ll << 31) || d->n_faces * d->B >= (1ll << 31))
        return set_error(NOF_EINVAL, "%s: n_faces=%lld must not be negative and B*n_faces must be below 2^31", fn,
                         (long long)d->n_faces);
    if (d->n_vertices < 0) return set_error(NOF_EINVAL, "%s: n_vertices=%lld must not be negative", fn, (long long)d->n_vertices);
    if (!(d->znear > 0)) return set_error(NOF_EINVAL, "%s: znear=%g must be > 0", fn, d->znear);
    if (!(d->zfar > d->znear)) return set_error(NOF_EINVAL, "%s: zfar=%g must be > znear=%g", fn, d->zfar, d->znear);
    if (d->small_max_pixels < 0)
        return set_error(NOF_EINVAL, "%s: small_max_pixels=%d must not be negative", fn, d->small_max_pixels);
    if (d->colour_mode != NOF_MESH_COLOUR_FLAT && d->colour_mode != NOF_MESH_COLOUR_VERTEX &&
        d->colour_mode != NOF_MESH_COLOUR_TEXTURE)
        return set_error(NOF_EINVAL, "%s: colour_mode=%d is not a NOF_MESH_COLOUR_* value", fn, d->colour_mode);
    if (d->colour_mode == NOF_MESH_COLOUR_VERTEX && !d->colors)
        return set_error(NOF_EINVAL, "%s: colour_mode vertex needs colors", fn);
    if (d->colour_mode == NOF_MESH_COLOUR_TEXTURE) {
        if (!d->uv) return set_error(NOF_EINVAL, "%s: colour_mode texture needs uv", fn);
        if (!d->texture) return set_error(NOF_EINVAL, "%s: colour_mode texture needs texture", fn);
        if (d->tex_h < 1 || d->tex_w < 1)
            return set_error(NOF_EINVAL, "%s: tex_h=%d, tex_w=%d must be positive", fn, d->tex_h, d->tex_w);
    }
    if (int rc = require_pointers(fn, {{d->vertices, "vertices", d->n_faces > 0}, {d->faces, "faces", d->n_faces > 0},
                                       {d->ob_in_cam, "ob_in_cam"}, {d->K, "K"}, {d->workspace, "workspace"},
                                       {d->depth, "depth"}, {d->face, "face"}, {d->rgb, "rgb"}, {d->normal, "normal"}}))
        return rc;
    const Pinhole c = {d->K[0], d->K[4], d->K[2], d->K[5]};
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_pixels = (int64_t)d->B * d->H * d->W, n_items = (int64_t)d->B * d->n_faces;
    unsigned int *n_large = (unsigned int *)d->workspace;
    unsigned long long *zbuf = (unsigned long long *)((char *)d->workspace + kMeshHead);
    unsigned long long *list = zbuf + n_pixels;
    if (hipMemsetAsync(n_large, 0, kMeshHead, s) != hipSuccess || hipMemsetAsync(zbuf, 0xff, (size_t)n_pixels * 8, s) != hipSuccess)
        return set_error(NOF_ELAUNCH, "%s: memset failed", fn);
    if (n_items > 0) {
        hipLaunchKernelGGL(k_mesh_setup, dim3(div_up(n_items, 256)), dim3(256), 0, s, d->vertices, d->faces, d->n_faces,
                           d->ob_in_cam, n_items, c, d->H, d->W, d->znear, d->zfar, d->small_max_pixels, zbuf, list, n_large);
        // 1024 blocks of 4 waves: every CU holds a few, and a list shorter than that leaves waves idle at once
        const uint32_t blocks = (uint32_t)(n_items < 4096 ? (n_items + 3) / 4 : 1024);
        hipLaunchKernelGGL(k_mesh_large, dim3(blocks), dim3(256), 0, s, d->vertices, d->faces, d->ob_in_cam, c, d->H, d->W,
                           d->znear, d->zfar, zbuf, list, n_large);
    }
    MeshShade sh = {d->colors, d->normals, d->uv, d->texture, d->tex_h, d->tex_w, d->colour_mode, d->shade,
                    {(double)d->base_rgb[0], (double)d->base_rgb[1], (double)d->base_rgb[2]}};
    hipLaunchKernelGGL(k_mesh_shade, dim3(div_up(n_pixels, 256)), dim3(256), 0, s, d->vertices, d->faces, d->ob_in_cam,
                       n_pixels, c, d->H, d->W, d->znear, d->zfar, sh, zbuf, d->depth, d->face, d->rgb, d->normal);
    return check_launch(fn);
}

}  // extern "C"
