// Frame maps (include/nof.h group 10): from raw depth frames to the point and normal maps, the 3-D
// matches and the covisibility counts that ransac_pairs and optimize_poses start from. The reference's
// Frame::processDepth, Frame::depthToCloudAndNormals and Frame::invalidatePixelsByMask over
// erodeDepthMap, gaussFilterDepthMap, convertDepthFloatToCameraSpaceFloat4, computeNormals and
// filterDepthSmoothedEdges (BundleTrack/src/cuda/CUDAImageUtil.cu), SiftManager::makeCorrespondence
// and computeCovisibility, batched over N frames.
//
// This comment is the definition; tests/frame_maps_oracle.py restates it in numpy float64. Depth is
// float32 metres, [N,H,W], pixel (u, v) = (column, row). Every load of a depth goes through
// clean(x) = x if x is finite, else 0. All arithmetic is IEEE float64 in the order written here,
// without contraction; a float32 input is widened exactly, an output is rounded once to float32.
// exp in the bilateral weight is the only operation that is not correctly rounded. Thresholds are
// the doubles of the descriptor. No floating-point atomics: the same bytes on every run.
//
//  k_frame_erode      d -> e. c = clean(d(u,v)). e = 0 unless c > depth_min and c <= zfar. Over the
//                     (2r+1)^2 window, a tap x = clean(d(u+j, v+i)) inside the image is bad if
//                     x < depth_min or |x - c| > diff; taps outside the image are not counted.
//                     e = 0 if (double)bad / (double)(2r+1)^2 >= ratio, else c.
//  k_frame_bilateral  e -> b. A tap x (inside the image, cleaned) is usable if depth_min <= x and
//                     x <= zfar. Taps are visited column by column: m = u-r .. u+r outer, n = v-r ..
//                     v+r inner. n_use = usable taps, S = their sum in that order; n_use == 0: b = 0.
//                     mean = S / n_use. A tap contributes if it is usable and |x - mean| < band:
//                     w = exp((-(double)((m-u)^2 + (n-v)^2) / two_sigma_d_sq)
//                             - ((c - x) (c - x)) / two_sigma_r_sq),   c = clean(e(u,v)) (it may be 0)
//                     sw = sw + w, s = s + w x in tap order from 0; b = s / sw if sw > 0, else 0.
//                     An invalid centre is filled from its neighbours, as in the reference.
//  k_frame_geometry   b, K, mask -> depth, points, normals, n_valid. z = clean(b(u,v));
//                     P(u,v) = (((u - cx) z) / fx, ((v - cy) z) / fy, z) if z >= depth_min, else
//                     (0,0,0): f64, not rounded. A neighbour q of the centre is near if z_q >=
//                     depth_min and |z_q - z| <= z_diff. Normal n: (0,0,0) on the image border and
//                     where z < depth_min. With D = (u, v+1), U = (u, v-1): row_dir = P_D - P_U if
//                     both are near, else P_D - P if D is near, else P_U - P if U is near, else n = 0.
//                     With R = (u+1, v), L = (u-1, v): col_dir likewise (P_R - P_L, P_R - P, P_L - P).
//                     a = row_dir, b = col_dir, m = (ay bz - az by, az bx - ax bz, ax by - ay bx),
//                     l = sqrt((mx mx + my my) + mz mz); n = 0 unless l > 0; n = m / l per component;
//                     if (nx (-Px) + ny (-Py)) + nz (-Pz) < 0 then n = -n.
//                     Keep: z >= depth_min, and mask(u,v) != 0 (when a mask is given), and, where
//                     n != 0, not |(nx Px/lp + ny Py/lp) + nz Pz/lp| < sin_edge with lp = sqrt((Px Px
//                     + Py Py) + Pz Pz). A kept pixel: depth = z (the float32 it was), points =
//                     f32(P), normals = f32(n). Any other pixel: zeros in all three. Every element
//                     is written. n_valid[f] = kept pixels of frame f (ballot, LDS, one integer
//                     atomicAdd per block; the call clears it first).
//  k_frame_lift       one lane per match row i of pair p (pair_start, the row layout of group 8),
//                     frames (fa, fb) = pair_frames[p]. ua = round(uv_a[i][0]) etc. with C round
//                     (half away from zero); the row is invalid unless all four coordinates are
//                     finite and 0 <= ua < W, 0 <= va < H (after rounding), the same for b, and
//                     both frames lie in 0 .. N-1. Pa, na, Pb, nb are the maps' float32 entries,
//                     widened. Invalid if Pa.z <= depth_min or Pb.z <= depth_min. With poses: A =
//                     xform_point(pose[fa], Pa), B likewise, d = sqrt((dx dx + dy dy) + dz dz),
//                     dx = Ax - Bx; with gate_dist the row is invalid unless d <= max_dist. With
//                     gate_normal: ma = xform_dir(pose[fa], na), la = sqrt((max max + may may) +
//                     maz maz), ha = ma / la, hb likewise; invalid unless (hax hbx + hay hby) +
//                     haz hbz >= cos_normal (a zero normal gives NaN and fails). A valid row holds
//                     Pa, Pb, na, nb in the frames' cameras; an invalid one zeros. No compaction.
//  k_frame_covis      pair q = (a, b), T = inv(pose_b) pose_a from the host. Pixels (u, v) of frame a
//                     with u, v multiples of stride. Visited: P.z >= depth_min and n != (0,0,0).
//                     p' = xform_point(T, P), n' = xform_dir(T, n), lp = sqrt((p'x p'x + p'y p'y) +
//                     p'z p'z), ln likewise; visible if ((-p'x / lp) (n'x / ln) + (-p'y / lp)
//                     (n'y / ln)) + (-p'z / lp) (n'z / ln) > cos_visible. counts[q] = (visible,
//                     total), integer adds only.
//
// Shape. erode and bilateral stage a (8 + 2r) x (32 + 2r) tile of cleaned depth per 32 x 8 block in
// LDS (r <= 8); a tap outside the image is staged as NaN, which fails every comparison above, so it
// is neither bad nor usable, while an invalid tap inside the image is staged as 0. geometry stages
// the tile with a halo of one pixel.
#include "geom_device.h"
#include "host_entry.h"

#pragma clang fp contract(off)

namespace nof {

constexpr int FM_BX = 32, FM_BY = 8;          // a block's pixels: 32 columns x 8 rows, one per thread
constexpr int FM_MAX_RADIUS = 8;
constexpr int FM_TW = FM_BX + 2 * FM_MAX_RADIUS + 1;      // row stride of the staged tile (odd)
constexpr int FM_TH = FM_BY + 2 * FM_MAX_RADIUS;

__device__ __forceinline__ float fm_clean(float x) { return fabsf(x) <= 3.402823466e38f ? x : 0.0f; }   // NaN, inf -> 0

// Stage the block's pixels plus a halo of r, cleaned; NaN outside the image.
__device__ __forceinline__ void fm_stage(float (*tile)[FM_TW], const float *__restrict__ img, int H, int W, int r) {
    const int u0 = (int)blockIdx.x * FM_BX - r, v0 = (int)blockIdx.y * FM_BY - r;
    const int tw = FM_BX + 2 * r, th = FM_BY + 2 * r;
    for (int i = threadIdx.y * FM_BX + threadIdx.x; i < tw * th; i += FM_BX * FM_BY) {
        const int ty = i / tw, tx = i - ty * tw;
        const int u = u0 + tx, v = v0 + ty;
        const bool in = u >= 0 && u < W && v >= 0 && v < H;
        tile[ty][tx] = in ? fm_clean(img[(size_t)v * W + u]) : __builtin_nanf("");
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_frame_erode(const float *__restrict__ in, float *__restrict__ out, int H, int W,
                                                     int r, double depth_min, double zfar, double diff, double ratio) {
    __shared__ float tile[FM_TH][FM_TW];
    const size_t frame = (size_t)blockIdx.z * H * W;
    fm_stage(tile, in + frame, H, W, r);
    const int u = blockIdx.x * FM_BX + threadIdx.x, v = blockIdx.y * FM_BY + threadIdx.y;
    if (u >= W || v >= H) return;
    const float cf = tile[threadIdx.y + r][threadIdx.x + r];
    const double c = cf;
    float res = 0.0f;
    if (c > depth_min && c <= zfar) {
        int bad = 0;
        for (int i = 0; i <= 2 * r; ++i)
            for (int j = 0; j <= 2 * r; ++j) {
                const double x = tile[threadIdx.y + i][threadIdx.x + j];      // NaN outside the image: not bad
                bad += (x < depth_min || fabs(x - c) > diff) ? 1 : 0;
            }
        const int side = 2 * r + 1;
        res = (double)bad / (double)(side * side) >= ratio ? 0.0f : cf;
    }
    out[frame + (size_t)v * W + u] = res;
}

__global__ __launch_bounds__(256) void k_frame_bilateral(const float *__restrict__ in, float *__restrict__ out, int H,
                                                         int W, int r, double depth_min, double zfar,
                                                         double two_sigma_d_sq, double two_sigma_r_sq, double band) {
    __shared__ float tile[FM_TH][FM_TW];
    const size_t frame = (size_t)blockIdx.z * H * W;
    fm_stage(tile, in + frame, H, W, r);
    const int u = blockIdx.x * FM_BX + threadIdx.x, v = blockIdx.y * FM_BY + threadIdx.y;
    if (u >= W || v >= H) return;
    const double c = tile[threadIdx.y + r][threadIdx.x + r];
    double S = 0.0;
    int n_use = 0;
    for (int j = 0; j <= 2 * r; ++j)             // columns outside, rows inside
        for (int i = 0; i <= 2 * r; ++i) {
            const double x = tile[threadIdx.y + i][threadIdx.x + j];
            if (depth_min <= x && x <= zfar) {
                n_use += 1;
                S += x;
            }
        }
    float res = 0.0f;
    if (n_use > 0) {
        const double mean = S / (double)n_use;
        double sw = 0.0, s = 0.0;
        for (int j = 0; j <= 2 * r; ++j)
            for (int i = 0; i <= 2 * r; ++i) {
                const double x = tile[threadIdx.y + i][threadIdx.x + j];
                if (depth_min <= x && x <= zfar && fabs(x - mean) < band) {
                    const int dx = j - r, dy = i - r;
                    const double w = exp((-(double)(dx * dx + dy * dy) / two_sigma_d_sq) - ((c - x) * (c - x)) / two_sigma_r_sq);
                    sw += w;
                    s += w * x;
                }
            }
        if (sw > 0.0) res = (float)(s / sw);
    }
    out[frame + (size_t)v * W + u] = res;
}

struct FmPoint {
    double x, y, z;
};

__device__ __forceinline__ FmPoint fm_point(int u, int v, double z, double fx, double fy, double cx, double cy,
                                            double depth_min) {
    FmPoint p = {0.0, 0.0, 0.0};
    if (z >= depth_min) {
        p.x = (((double)u - cx) * z) / fx;
        p.y = (((double)v - cy) * z) / fy;
        p.z = z;
    }
    return p;
}

// One direction of the normal's stencil: the central difference, else forward, else backward. False if none applies.
__device__ __forceinline__ bool fm_dir(const FmPoint &c, const FmPoint &plus, const FmPoint &minus, double depth_min,
                                       double z_diff, double (&d)[3]) {
    const bool np = plus.z >= depth_min && fabs(plus.z - c.z) <= z_diff;
    const bool nm = minus.z >= depth_min && fabs(minus.z - c.z) <= z_diff;
    if (np && nm) {
        d[0] = plus.x - minus.x, d[1] = plus.y - minus.y, d[2] = plus.z - minus.z;
    } else if (np) {
        d[0] = plus.x - c.x, d[1] = plus.y - c.y, d[2] = plus.z - c.z;
    } else if (nm) {
        d[0] = minus.x - c.x, d[1] = minus.y - c.y, d[2] = minus.z - c.z;
    } else {
        return false;
    }
    return true;
}

__global__ __launch_bounds__(256) void k_frame_geometry(const float *__restrict__ in, const double *__restrict__ K4,
                                                        const uint8_t *__restrict__ mask, int H, int W, double depth_min,
                                                        double z_diff, double sin_edge, float *__restrict__ depth,
                                                        float *__restrict__ points, float *__restrict__ normals,
                                                        int32_t *__restrict__ n_valid) {
    __shared__ float tile[FM_TH][FM_TW];
    __shared__ int32_t wave_count[4];
    const int f = blockIdx.z;
    const size_t frame = (size_t)f * H * W;
    fm_stage(tile, in + frame, H, W, 1);
    const int u = blockIdx.x * FM_BX + threadIdx.x, v = blockIdx.y * FM_BY + threadIdx.y;
    const bool inside = u < W && v < H;
    bool keep = false;
    if (inside) {
        const double fx = K4[f * 4], fy = K4[f * 4 + 1], cx = K4[f * 4 + 2], cy = K4[f * 4 + 3];
        const int ty = threadIdx.y + 1, tx = threadIdx.x + 1;
        const float zf = tile[ty][tx];
        const FmPoint P = fm_point(u, v, zf, fx, fy, cx, cy, depth_min);
        double n[3] = {0.0, 0.0, 0.0};
        keep = (double)zf >= depth_min;
        if (keep && u > 0 && u < W - 1 && v > 0 && v < H - 1) {
            const FmPoint D = fm_point(u, v + 1, tile[ty + 1][tx], fx, fy, cx, cy, depth_min);
            const FmPoint U = fm_point(u, v - 1, tile[ty - 1][tx], fx, fy, cx, cy, depth_min);
            const FmPoint R = fm_point(u + 1, v, tile[ty][tx + 1], fx, fy, cx, cy, depth_min);
            const FmPoint L = fm_point(u - 1, v, tile[ty][tx - 1], fx, fy, cx, cy, depth_min);
            double a[3], b[3];
            if (fm_dir(P, D, U, depth_min, z_diff, a) && fm_dir(P, R, L, depth_min, z_diff, b)) {
                const double mx = a[1] * b[2] - a[2] * b[1], my = a[2] * b[0] - a[0] * b[2], mz = a[0] * b[1] - a[1] * b[0];
                const double l = sqrt((mx * mx + my * my) + mz * mz);
                if (l > 0.0) {
                    n[0] = mx / l, n[1] = my / l, n[2] = mz / l;
                    if ((n[0] * (-P.x) + n[1] * (-P.y)) + n[2] * (-P.z) < 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
                }
            }
        }
        if (keep && (n[0] != 0.0 || n[1] != 0.0 || n[2] != 0.0)) {
            const double lp = sqrt((P.x * P.x + P.y * P.y) + P.z * P.z);
            const double dot = (n[0] * (P.x / lp) + n[1] * (P.y / lp)) + n[2] * (P.z / lp);
            if (fabs(dot) < sin_edge) keep = false;
        }
        const size_t pix = frame + (size_t)v * W + u;
        if (keep && mask && mask[pix] == 0) keep = false;
        depth[pix] = keep ? zf : 0.0f;
        points[pix * 3] = keep ? (float)P.x : 0.0f;
        points[pix * 3 + 1] = keep ? (float)P.y : 0.0f;
        points[pix * 3 + 2] = keep ? (float)P.z : 0.0f;
        normals[pix * 3] = keep ? (float)n[0] : 0.0f;
        normals[pix * 3 + 1] = keep ? (float)n[1] : 0.0f;
        normals[pix * 3 + 2] = keep ? (float)n[2] : 0.0f;
    }
    // every thread of the block arrives here
    const int tid = threadIdx.y * FM_BX + threadIdx.x;
    const int32_t in_wave = (int32_t)__popcll(__ballot(keep));
    if ((tid & 63) == 0) wave_count[tid >> 6] = in_wave;
    __syncthreads();
    if (tid == 0) {
        const int32_t total = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
        if (total) atomicAdd(&n_valid[f], total);
    }
}

// The cleaned, rounded pixel of one match coordinate pair; false if it is not a pixel of the image.
__device__ __forceinline__ bool fm_pixel(double uf, double vf, int H, int W, int &u, int &v) {
    if (!(fabs(uf) <= 1.7976931348623157e308) || !(fabs(vf) <= 1.7976931348623157e308)) return false;
    const double ur = round(uf), vr = round(vf);       // half away from zero
    if (!(ur >= 0.0 && ur < (double)W && vr >= 0.0 && vr < (double)H)) return false;
    u = (int)ur, v = (int)vr;
    return true;
}

__device__ __forceinline__ void fm_load3(const float *__restrict__ map, size_t pix, double (&o)[3]) {
    o[0] = map[pix * 3], o[1] = map[pix * 3 + 1], o[2] = map[pix * 3 + 2];
}

__global__ __launch_bounds__(256) void k_frame_lift(nof_frame_lift_desc d) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= d.M) return;
    // the pair of row i: the last p with pair_start[p] <= i (empty pairs share a start with their successor)
    int lo = 0, hi = d.P;                     // invariant: pair_start[lo] <= i, the answer is in [lo, hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)d.pair_start[mid] <= i) lo = mid; else hi = mid;
    }
    const int fa = d.pair_frames[lo * 2], fb = d.pair_frames[lo * 2 + 1];
    double Pa[3] = {0, 0, 0}, Pb[3] = {0, 0, 0}, na[3] = {0, 0, 0}, nb[3] = {0, 0, 0};
    int ua, va, ub, vb;
    bool ok = fa >= 0 && fa < d.N && fb >= 0 && fb < d.N;
    ok = ok && fm_pixel(d.uv_a[i * 2], d.uv_a[i * 2 + 1], d.H, d.W, ua, va);
    ok = ok && fm_pixel(d.uv_b[i * 2], d.uv_b[i * 2 + 1], d.H, d.W, ub, vb);
    if (ok) {
        const size_t pa = ((size_t)fa * d.H + va) * d.W + ua, pb = ((size_t)fb * d.H + vb) * d.W + ub;
        fm_load3(d.points, pa, Pa);
        fm_load3(d.points, pb, Pb);
        fm_load3(d.normals, pa, na);
        fm_load3(d.normals, pb, nb);
        ok = !(Pa[2] <= d.depth_min) && !(Pb[2] <= d.depth_min);
    }
    if (ok && d.poses) {
        const double *Ta = d.poses + (size_t)fa * 16, *Tb = d.poses + (size_t)fb * 16;
        if (d.gate_dist) {
            double A[3], B[3];
            xform_point(Ta, Pa[0], Pa[1], Pa[2], A);
            xform_point(Tb, Pb[0], Pb[1], Pb[2], B);
            const double dx = A[0] - B[0], dy = A[1] - B[1], dz = A[2] - B[2];
            ok = sqrt((dx * dx + dy * dy) + dz * dz) <= d.max_dist;
        }
        if (ok && d.gate_normal) {
            double ma[3], mb[3];
            xform_dir(Ta, na[0], na[1], na[2], ma);
            xform_dir(Tb, nb[0], nb[1], nb[2], mb);
            const double la = sqrt((ma[0] * ma[0] + ma[1] * ma[1]) + ma[2] * ma[2]);
            const double lb = sqrt((mb[0] * mb[0] + mb[1] * mb[1]) + mb[2] * mb[2]);
            const double dot = ((ma[0] / la) * (mb[0] / lb) + (ma[1] / la) * (mb[1] / lb)) + (ma[2] / la) * (mb[2] / lb);
            ok = dot >= d.cos_normal;          // NaN (a zero normal) fails
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d.pts_a[i * 3 + k] = ok ? Pa[k] : 0.0;
        d.pts_b[i * 3 + k] = ok ? Pb[k] : 0.0;
        d.normals_a[i * 3 + k] = ok ? na[k] : 0.0;
        d.normals_b[i * 3 + k] = ok ? nb[k] : 0.0;
    }
    d.valid[i] = ok ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_frame_covis(const float *__restrict__ points, const float *__restrict__ normals,
                                                     int N, int H, int W, const int32_t *__restrict__ pairs,
                                                     const double *__restrict__ T16, int stride, int ws, int n_pix,
                                                     double depth_min, double cos_visible, int32_t *__restrict__ counts) {
    __shared__ int32_t wave_count[4][2];
    const int q = blockIdx.y;
    const int fa = pairs[q * 2];
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool visited = false, visible = false;
    if (i < n_pix && fa >= 0 && fa < N) {
        const int v = (i / ws) * stride, u = (i - (i / ws) * ws) * stride;       // v < H, u < W by the host's ws, n_pix
        const size_t pix = ((size_t)fa * H + v) * W + u;
        double P[3], n[3];
        fm_load3(points, pix, P);
        fm_load3(normals, pix, n);
        visited = P[2] >= depth_min && (n[0] != 0.0 || n[1] != 0.0 || n[2] != 0.0);
        if (visited) {
            const double *T = T16 + (size_t)q * 16;
            double p2[3], n2[3];
            xform_point(T, P[0], P[1], P[2], p2);
            xform_dir(T, n[0], n[1], n[2], n2);
            const double lp = sqrt((p2[0] * p2[0] + p2[1] * p2[1]) + p2[2] * p2[2]);
            const double ln = sqrt((n2[0] * n2[0] + n2[1] * n2[1]) + n2[2] * n2[2]);
            const double dot = ((-p2[0] / lp) * (n2[0] / ln) + (-p2[1] / lp) * (n2[1] / ln)) + (-p2[2] / lp) * (n2[2] / ln);
            visible = dot > cos_visible;
        }
    }
    const int32_t vis = (int32_t)__popcll(__ballot(visible)), tot = (int32_t)__popcll(__ballot(visited));
    if ((threadIdx.x & 63) == 0) {
        wave_count[threadIdx.x >> 6][0] = vis;
        wave_count[threadIdx.x >> 6][1] = tot;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        const int32_t total = (wave_count[0][k] + wave_count[1][k]) + (wave_count[2][k] + wave_count[3][k]);
        if (total) atomicAdd(&counts[q * 2 + k], total);
    }
}

// The image shape shared by the five calls: N, H, W at least 1 and N H W below 2^31.
static int fm_check_shape(const char *fn, int32_t N, int32_t H, int32_t W) {
    if (N < 1 || N > 65535) return set_error(NOF_EINVAL, "%s: N=%d must be in 1..65535", fn, N);
    if (H < 1 || W < 1) return set_error(NOF_EINVAL, "%s: H=%d, W=%d must be at least 1", fn, H, W);
    if ((int64_t)N * H * W >= (1ll << 31))
        return set_error(NOF_EINVAL, "%s: N*H*W=%lld must be below 2^31", fn, (long long)N * H * W);
    if (div_up(H, FM_BY) > 65535) return set_error(NOF_EINVAL, "%s: H=%d must be at most %d", fn, H, 65535 * FM_BY);
    return NOF_OK;
}

static dim3 fm_grid(int32_t N, int32_t H, int32_t W) { return dim3(div_up(W, FM_BX), div_up(H, FM_BY), (unsigned)N); }

}  // namespace nof

using namespace nof;

extern "C" {

int nof_frame_erode(const nof_frame_erode_desc *d, void *stream) {
    const char *fn = "frame_erode";
    if (!d) return set_error(NOF_EINVAL, "%s: desc is NULL", fn);
    if (int rc = fm_check_shape(fn, d->N, d->H, d->W)) return rc;
    if (d->radius < 0 || d->radius > FM_MAX_RADIUS)
        return set_error(NOF_EINVAL, "%s: radius=%d must be in 0..%d", fn, d->radius, FM_MAX_RADIUS);
    if (!d->in) return set_error(NOF_EINVAL, "%s: in is NULL", fn);
    if (!d->out) return set_error(NOF_EINVAL, "%s: out is NULL", fn);
    if (d->in == d->out) return set_error(NOF_EINVAL, "%s: in and out are the same buffer", fn);
    if (d->depth_min != d->depth_min || d->zfar != d->zfar || d->diff != d->diff || d->ratio != d->ratio)
        return set_error(NOF_EINVAL, "%s: depth_min, zfar, diff or ratio is NaN", fn);
    hipLaunchKernelGGL(k_frame_erode, fm_grid(d->N, d->H, d->W), dim3(FM_BX, FM_BY), 0, (hipStream_t)stream, d->in, d->out,
                       d->H, d->W, d->radius, d->depth_min, d->zfar, d->diff, d->ratio);
    return check_launch(fn);
}

int nof_frame_bilateral(const nof_frame_bilateral_desc *d, void *stream) {
    const char *fn = "frame_bilateral";
    if (!d) return set_error(NOF_EINVAL, "%s: desc is NULL", fn);
    if (int rc = fm_check_shape(fn, d->N, d->H, d->W)) return rc;
    if (d->radius < 0 || d->radius > FM_MAX_RADIUS)
        return set_error(NOF_EINVAL, "%s: radius=%d must be in 0..%d", fn, d->radius, FM_MAX_RADIUS);
    if (!d->in) return set_error(NOF_EINVAL, "%s: in is NULL", fn);
    if (!d->out) return set_error(NOF_EINVAL, "%s: out is NULL", fn);
    if (d->in == d->out) return set_error(NOF_EINVAL, "%s: in and out are the same buffer", fn);
    if (!(d->two_sigma_d_sq > 0) || !(d->two_sigma_r_sq > 0))
        return set_error(NOF_EINVAL, "%s: two_sigma_d_sq=%g and two_sigma_r_sq=%g must be positive", fn, d->two_sigma_d_sq,
                         d->two_sigma_r_sq);
    if (d->depth_min != d->depth_min || d->zfar != d->zfar || d->band != d->band)
        return set_error(NOF_EINVAL, "%s: depth_min, zfar or band is NaN", fn);
    hipLaunchKernelGGL(k_frame_bilateral, fm_grid(d->N, d->H, d->W), dim3(FM_BX, FM_BY), 0, (hipStream_t)stream, d->in,
                       d->out, d->H, d->W, d->radius, d->depth_min, d->zfar, d->two_sigma_d_sq, d->two_sigma_r_sq, d->band);
    return check_launch(fn);
}

int nof_frame_geometry(const nof_frame_geometry_desc *d, void *stream) {
    const char *fn = "frame_geometry";
    if (!d) return set_error(NOF_EINVAL, "%s: desc is NULL", fn);
    if (int rc = fm_check_shape(fn, d->N, d->H, d->W)) return rc;
    if (int rc = require_pointers(fn, {{d->depth_in, "depth_in"}, {d->K, "K"}, {d->depth, "depth"}, {d->points, "points"},
                                       {d->normals, "normals"}, {d->n_valid, "n_valid"}}))
        return rc;
    if (d->depth_in == d->depth) return set_error(NOF_EINVAL, "%s: depth_in and depth are the same buffer", fn);
    if (d->depth_min != d->depth_min || d->z_diff != d->z_diff || d->sin_edge != d->sin_edge)
        return set_error(NOF_EINVAL, "%s: depth_min, z_diff or sin_edge is NaN", fn);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d->n_valid, 0, sizeof(int32_t) * (size_t)d->N, s) != hipSuccess)
        return set_error(NOF_ELAUNCH, "%s: memset failed", fn);
    hipLaunchKernelGGL(k_frame_geometry, fm_grid(d->N, d->H, d->W), dim3(FM_BX, FM_BY), 0, s, d->depth_in, d->K, d->mask,
                       d->H, d->W, d->depth_min, d->z_diff, d->sin_edge, d->depth, d->points, d->normals, d->n_valid);
    return check_launch(fn);
}

int nof_frame_lift_matches(const nof_frame_lift_desc *d, void *stream) {
    const char *fn = "frame_lift_matches";
    if (!d) return set_error(NOF_EINVAL, "%s: desc is NULL", fn);
    if (int rc = fm_check_shape(fn, d->N, d->H, d->W)) return rc;
    if (d->P < 1 || d->P > 65535) return set_error(NOF_EINVAL, "%s: P=%d must be in 1..65535", fn, d->P);
    if (d->M < 0 || d->M >= (1ll << 31))
        return set_error(NOF_EINVAL, "%s: M=%lld must be in 0..2^31-1", fn, (long long)d->M);
    if ((d->gate_dist || d->gate_normal) && !d->poses)
        return set_error(NOF_EINVAL, "%s: poses is NULL while a gate is on", fn);
    if (d->gate_dist && d->max_dist != d->max_dist) return set_error(NOF_EINVAL, "%s: max_dist is NaN", fn);
    if (d->gate_normal && d->cos_normal != d->cos_normal) return set_error(NOF_EINVAL, "%s: cos_normal is NaN", fn);
    if (d->depth_min != d->depth_min) return set_error(NOF_EINVAL, "%s: depth_min is NaN", fn);
    const bool rows = d->M > 0;
    if (int rc = require_pointers(fn, {{d->points, "points"}, {d->normals, "normals"}, {d->pair_frames, "pair_frames"},
                                       {d->pair_start, "pair_start"}, {d->uv_a, "uv_a", rows}, {d->uv_b, "uv_b", rows},
                                       {d->pts_a, "pts_a", rows}, {d->pts_b, "pts_b", rows},
                                       {d->normals_a, "normals_a", rows}, {d->normals_b, "normals_b", rows},
                                       {d->valid, "valid", rows}}))
        return rc;
    if (!rows) return NOF_OK;
    hipLaunchKernelGGL(k_frame_lift, dim3(div_up((uint64_t)d->M, 256)), dim3(256), 0, (hipStream_t)stream, *d);
    return check_launch(fn);
}

int nof_frame_covisibility(const nof_frame_covis_desc *d, void *stream) {
    const char *fn = "frame_covisibility";
    if (!d) return set_error(NOF_EINVAL, "%s: desc is NULL", fn);
    if (int rc = fm_check_shape(fn, d->N, d->H, d->W)) return rc;
    if (d->Q < 0 || d->Q > 65535) return set_error(NOF_EINVAL, "%s: Q=%d must be in 0..65535", fn, d->Q);
    if (d->stride < 1) return set_error(NOF_EINVAL, "%s: stride=%d must be at least 1", fn, d->stride);
    if (d->depth_min != d->depth_min || d->cos_visible != d->cos_visible)
        return set_error(NOF_EINVAL, "%s: depth_min or cos_visible is NaN", fn);
    if (int rc = require_pointers(fn, {{d->points, "points"}, {d->normals, "normals"}, {d->pairs, "pairs", d->Q > 0},
                                       {d->T, "T", d->Q > 0}, {d->counts, "counts", d->Q > 0}}))
        return rc;
    if (d->Q == 0) return NOF_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d->counts, 0, sizeof(int32_t) * 2 * (size_t)d->Q, s) != hipSuccess)
        return set_error(NOF_ELAUNCH, "%s: memset failed", fn);
    const int ws = (d->W + d->stride - 1) / d->stride, hs = (d->H + d->stride - 1) / d->stride;
    const int n_pix = ws * hs;              // <= H W < 2^31
    hipLaunchKernelGGL(k_frame_covis, dim3(div_up(n_pix, 256), (unsigned)d->Q), dim3(256), 0, s, d->points, d->normals, d->N,
                       d->H, d->W, d->pairs, d->T, d->stride, ws, n_pix, d->depth_min, d->cos_visible, d->counts);
    return check_launch(fn);
}

}  // extern "C"
