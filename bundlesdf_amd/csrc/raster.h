// The triangle raster shared by nof_raster_faces (texture.hip) and nof_render_mesh (mesh_render.hip):
// projection, cull, coverage, depth and the z-buffer key. The definition, all IEEE f64 + - * / in the
// stated order without contraction (oracle/texture.py's raster restates it in numpy):
//
//  project_face   per vertex (x, y, w) of the face, with the pose T = rows of [R | t] (object in camera,
//                 OpenCV): (X, Y, Z) = xform_point(T, x, y, w). A vertex at Z <= znear drops the face (no
//                 near-plane clipping). u = fx X / Z + cx, v = fy Y / Z + cy.
//                 area = (u1 - u0)(v2 - v0) - (u2 - u0)(v1 - v0); area == 0 drops the face. The bounding
//                 box is ceil(min) .. floor(max) per axis, clamped to the image; the comparisons are made
//                 in f64 before the cast, so a projection far outside the image (a vertex just beyond
//                 znear reaches past 2^31 pixels) or a non-finite one never meets an out-of-range
//                 double -> int conversion. A box that misses the image drops the face.
//  cover          at the pixel centre (px, py): e_k = the edge function of the edge opposite vertex k
//                 over the area (either orientation, edges inclusive), all three >= 0;
//                 zi = 1 / ((e0 / z0 + e1 / z1) + e2 / z2), kept where zi <= zfar.
//  splat          atomicMin of (bits of (float)zi << 32 | face) into the 64-bit z-buffer: depth and face
//                 id at once, the nearest face wins, the lowest face index among equal depths. An
//                 untouched pixel keeps all ones.
#pragma once
#include <cmath>

#include "geom_device.h"

#pragma clang fp contract(off)

namespace nof {

struct Pinhole {
    double fx, fy, cx, cy;
};

struct Tri {
    double u[3], v[3], z[3], area;
    int u0, u1, v0, v1;        // clamped bounding box, never empty
};

// T: the pose's rows of [R | t], row stride 4 (device memory or a kernel argument). False: the face is dropped.
__device__ __forceinline__ bool project_face(const float *__restrict__ V, const int64_t *__restrict__ F, int64_t f,
                                             const double *__restrict__ T, const Pinhole &c, int H, int W,
                                             double znear, Tri &t) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float *p = V + F[f * 3 + k] * 3;
        double X[3];
        xform_point(T, p[0], p[1], p[2], X);
        if (!(X[2] > znear)) return false;
        t.z[k] = X[2];
        t.u[k] = c.fx * X[0] / X[2] + c.cx;
        t.v[k] = c.fy * X[1] / X[2] + c.cy;
    }
    const double *u = t.u, *v = t.v;
    t.area = (u[1] - u[0]) * (v[2] - v[0]) - (u[2] - u[0]) * (v[1] - v[0]);
    if (t.area == 0.0) return false;
    const double lu = ceil(fmin(fmin(u[0], u[1]), u[2])), hu = floor(fmax(fmax(u[0], u[1]), u[2]));
    const double lv = ceil(fmin(fmin(v[0], v[1]), v[2])), hv = floor(fmax(fmax(v[0], v[1]), v[2]));
    if (!(lu <= (double)(W - 1)) || !(hu >= 0.0) || !(lv <= (double)(H - 1)) || !(hv >= 0.0)) return false;
    t.u0 = lu < 0.0 ? 0 : (int)lu;
    t.v0 = lv < 0.0 ? 0 : (int)lv;
    t.u1 = hu > (double)(W - 1) ? W - 1 : (int)hu;
    t.v1 = hv > (double)(H - 1) ? H - 1 : (int)hv;
    return true;
}

// Coverage and depth at pixel centre (px, py). False: not covered or beyond zfar.
__device__ __forceinline__ bool cover(const Tri &t, int px, int py, double zfar, double e[3], double &zi) {
    const double X = px, Y = py;
    const double *u = t.u, *v = t.v;
    // barycentric weights of vertex k = edge function of the opposite edge / area
    e[0] = ((u[2] - u[1]) * (Y - v[1]) - (v[2] - v[1]) * (X - u[1])) / t.area;
    e[1] = ((u[0] - u[2]) * (Y - v[2]) - (v[0] - v[2]) * (X - u[2])) / t.area;
    e[2] = ((u[1] - u[0]) * (Y - v[0]) - (v[1] - v[0]) * (X - u[0])) / t.area;
    if (e[0] < 0.0 || e[1] < 0.0 || e[2] < 0.0) return false;
    zi = 1.0 / ((e[0] / t.z[0] + e[1] / t.z[1]) + e[2] / t.z[2]);
    return zi <= zfar;
}

__device__ __forceinline__ void splat(const Tri &t, int px, int py, double zfar, uint32_t f, int W,
                                      unsigned long long *__restrict__ zb) {
    double e[3], zi;
    if (!cover(t, px, py, zfar, e, zi)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint((float)zi) << 32) | (unsigned long long)f;
    atomicMin(&zb[(size_t)py * W + px], key);
}

}  // namespace nof
