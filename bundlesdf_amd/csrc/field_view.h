// Free-camera surface render (nof_render_view): depth, normal and colour of the field's zero level
// set from any pose — no pool ray, no frame depth. It uses ray_trace.h's trace_ray_emit, field_core.h's
// encode_level and mlp_sdf_net and field_query.h's query_tile as they are. Forward only: nothing is
// written but the outputs and the call's own workspace.
//
// Per pixel, all in fp32 with every written operation rounded on its own (contraction off, correctly
// rounded division and square root), so that a float32 restatement on the host (tests/view_oracle.py)
// reproduces every position bit for bit:
//  1. ray: dir_cam = ((u - cx) / fx, -((v - cy) / fy), -1) as the pool stores it, v^ = dir_cam / |dir_cam|,
//     o = c2w[:3,3], d = R v^ (k_trace's expression); no pose-array correction.
//  2. trace: trace_ray_emit over the occupancy grid, at most Kmax intervals; an interval's entry is
//     clamped to t >= 0 (a camera inside an occupied voxel). T = sum of (t_out - t_in) in trace order.
//  3. coarse march: step_eff = max(step, T / max_steps), n = ceil(T / step_eff); sample k at occupied
//     length u_k = (k + 0.5) step_eff, mapped to t_k by the occupied-voxel sampler's walk (rem = u_k;
//     per interval: rem <= len ? t = t_in + rem : rem -= len); a u_k past the walked length reads the
//     last interval's exit. x = o + t_k d, SDF by k_query_sdf's tile (clip to [-1,1], same bits).
//  4. crossing: the first k with sdf_k <= 0; k = 0: t* = t_0; else the bracket [t_{k-1}, t_k].
//  5. refine: n_refine bisections (mid = 0.5 (lo + hi); sdf_mid > 0 moves lo, else hi), then
//     t* = lo + (hi - lo) sdf_lo / (sdf_lo - sdf_hi). Occupancy is not consulted.
//  6. outputs at x* = o + t* d: t*, depth = t* |v^_z|, normal = query_field's gradient / its norm
//     (zero stays zero), rgb = sigmoid(colour net on [geo(x*), sh3(d), frame features]) with
//     k_query_field's colour pass (run_network's zero-embedding rule, the amp rounding).
//
// Kernels:
//  * k_view_trace: a thread per ray (k_trace's shape: the DDA is serial per ray) — the ray record
//    (d, |v^_z|, T, interval count) and the interval list, in the call's workspace.
//  * k_view_march: a wave per ray, 4 waves per block, the sigma net's 8 fragments and the bias image
//    staged in LDS once per block. The wave walks the ray's samples front to back in tiles of 32 (one
//    sample per lane, the levels split over the two lane halves as in k_query_sdf) and stops at the
//    first tile with a crossing. One 32-B bracket record per ray.
//  * k_view_shade: a wave per 32 rays (misses masked), all 46 fragments staged as in k_query_field:
//    the bisection loop (k_query_sdf's tile per step), then query_tile at x* with the view direction.
//    A tile without a hit writes its zeros and leaves.
//
// Per ray at L = 16, amp: the march reads <= 32 x 16 levels x 4 corner-pair loads of 8 B per tile
// (16 KB, mostly L2 hits: neighbouring samples share cells) and its interval list (8 B per interval)
// once per tile; 2 x (32 x 64 + 64 x 16) = 6.1 KFLOP per sample, 197 K per tile. A hit adds n_refine
// + 1 point evaluations (1 / 32 of a tile each), the gradient's two backward layers (6.1 K) and the
// colour net (14.3 K). Records: 32 B ray + 8 B per interval + 32 B bracket written and read once;
// outputs 37 B.
#pragma once
#include "field_core.h"
#include "field_query.h"

// every operation of the positions rounds on its own: plain operators with contraction off (HIP's
// __fmul_rn / __fadd_rn are inline wrappers compiled under the default mode: their product and sum may
// still fuse into an FMA after inlining, so they are not used)
#pragma clang fp contract(off)

namespace nof {

constexpr int VRAY = 8, VBRK = 8;
enum { VF_MISS = 0, VF_BRACKET = 1, VF_INSIDE = 2 };
constexpr int VIEW_NFR = FR_L3;   // the sigma net's fragments: FR_L1 .. FR_L3 - 1

struct ViewArgs {
    float c2w[12];            // rows 0..2 of the camera-to-world matrix (normalised space)
    float fx, fy, cx, cy;
    int W;
    const int32_t *pixels;    // [n] row-major pixel index (v W + u) or null: ray i is pixel pixel0 + i
    int pixel0;
    int n;                    // rays of this launch
    float step;
    int max_steps, n_refine;
    const uint8_t *occ;       // [N^3] occupancy, x fastest
    int N, Kmax;
    const float *ff;          // the frame's feature row (n_ff floats) or null
    int n_ff;
    float *vray;              // [n][VRAY]: d, |v^_z|, T, interval count (workspace)
    float *iv;                // [n][Kmax][2] (t_in, t_out) (workspace)
    float *brk;               // [n][VBRK]: t_lo, t_hi, sdf_lo, sdf_hi, flag, k, tiles marched (workspace)
    float *t, *depth, *normal, *rgb;
    uint8_t *hit;
    int32_t *index, *tiles;   // optional: the coarse crossing sample k (-1: none), tiles marched
};

__device__ __forceinline__ void view_point(const ViewArgs &v, const float d[3], float t, float x[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = v.c2w[4 * c + 3] + t * d[c];
}

// SDF of a tile of 32 points in k_query_sdf's instruction order (the same bits); on = the lane holds a point
template <typename TM, typename TT>
__device__ __forceinline__ float tile_sdf(const FieldArgs &a, const LdsW<TM> &W, const float *s_b, float x[3], bool on,
                                          int lane) {
    const int h = lane >> 5;
#pragma unroll
    for (int d = 0; d < 3; ++d) x[d] = fminf(fmaxf(x[d], -1.f), 1.f);   // torch.clip(inputs, -1, 1)
    const float x01[3] = {(x[0] + 1) / 2, (x[1] + 1) / 2, (x[2] + 1) / 2};
    Acts<TM> A;
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int lv = lane_level(ss, qq, h);
            float f[2] = {0.f, 0.f};
            if (on && lv < (int)a.L) encode_level<TT>(a, level_info(a, lv), x01, f);
            frag_set<TM>(A.X[ss], 2 * qq, f[0]);
            frag_set<TM>(A.X[ss], 2 * qq + 1, f[1]);
        }
    }
    float sdf;
    f16v l2;
    mlp_sdf_net<TM>(W, s_b, A, lane, sdf, l2);
    return sdf;
}

__global__ __launch_bounds__(256) void k_view_trace(ViewArgs v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v.n) return;
    const int pix = v.pixels ? v.pixels[i] : v.pixel0 + i;
    const int pu = pix % v.W, pv = pix / v.W;
    // camera_dir (ray_pool.hip) and k_trace's normalisation and rotation
    const float dc[3] = {((float)pu - v.cx) / v.fx, -(((float)pv - v.cy) / v.fy), -1.0f};
    const float nrm = sqrtf((dc[0] * dc[0] + dc[1] * dc[1]) + dc[2] * dc[2]);
    const float vd[3] = {dc[0] / nrm, dc[1] / nrm, dc[2] / nrm};
    const float o[3] = {v.c2w[3], v.c2w[7], v.c2w[11]};
    float d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = (v.c2w[c * 4] * vd[0] + v.c2w[c * 4 + 1] * vd[1]) + v.c2w[c * 4 + 2] * vd[2];
    float *dst = v.iv + (size_t)i * v.Kmax * 2;
    float total = 0.f;
    const int k = trace_ray_emit(v.occ, v.N, o, d, v.Kmax, [&](int j, float tin, float tout) {
        tin = fmaxf(tin, 0.f);
        *reinterpret_cast<float2 *>(dst + j * 2) = make_float2(tin, tout);
        total = total + (tout - tin);
    });
    float4 *rec = reinterpret_cast<float4 *>(v.vray + (size_t)i * VRAY);
    rec[0] = make_float4(d[0], d[1], d[2], fabsf(vd[2]));
    rec[1] = make_float4(total, __int_as_float(k), 0.f, 0.f);
}

template <typename TM, typename TT>
__global__ __launch_bounds__(256) void k_view_march(FieldArgs a, ViewArgs v) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    TM *s_fr = reinterpret_cast<TM *>(smem);
    float *s_b = staged_bias<TM, VIEW_NFR>(smem);
    NOF_STAGE_FRAGS(TM, VIEW_NFR, 0, false, a, smem, s_b);
    __syncthreads();
    const int lane = threadIdx.x & 63, n = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const LdsW<TM> W{s_fr};
    for (int ray = (int)blockIdx.x * 4 + wave; ray < v.n; ray += (int)gridDim.x * 4) {
        const float4 *rec = reinterpret_cast<const float4 *>(v.vray + (size_t)ray * VRAY);
        const float4 r0 = rec[0], r1 = rec[1];
        const float d[3] = {r0.x, r0.y, r0.z};
        const float T = r1.x;
        const int cnt = __builtin_amdgcn_readfirstlane(__float_as_int(r1.y));
        const float2 *iv = reinterpret_cast<const float2 *>(v.iv + (size_t)ray * v.Kmax * 2);
        int flag = VF_MISS, kc = -1, tiles = 0;
        float tlo = 0.f, thi = 0.f, slo = 0.f, shi = 0.f;
        if (cnt > 0 && T > 0.f) {
            const float step_eff = fmaxf(v.step, T / (float)v.max_steps);
            const int ns = __builtin_amdgcn_readfirstlane((int)ceilf(T / step_eff));
            const float t_end = iv[cnt - 1].y;
            float prev_t = 0.f, prev_s = 0.f;
            for (int tile = 0; tile * 32 < ns; ++tile) {
                const int k = tile * 32 + n;
                const bool on = k < ns;
                // the occupied-voxel sampler's walk (sample_z): sequential subtraction over the intervals
                float rem = ((float)k + 0.5f) * step_eff, t = t_end;
                bool done = !on;
                for (int i = 0; i < cnt; ++i) {
                    const float2 io = iv[i];
                    const float len = io.y - io.x;
                    const bool here = !done && rem <= len;
                    t = here ? io.x + rem : t;
                    rem = done || here ? rem : rem - len;
                    done = done || here;
                    if (!__any(!done)) break;
                }
                float x[3];
                view_point(v, d, t, x);
                const float sdf = tile_sdf<TM, TT>(a, W, s_b, x, on, lane);
                ++tiles;
                // both lane halves hold the same 32 samples: the lower half's bits
                const uint32_t neg = (uint32_t)__ballot(on && sdf <= 0.f);
                if (neg) {
                    const int j = __builtin_ctz(neg);
                    kc = tile * 32 + j;
                    thi = __shfl(t, j, 64);
                    shi = __shfl(sdf, j, 64);
                    const float tb = __shfl(t, (j + 31) & 31, 64), sb = __shfl(sdf, (j + 31) & 31, 64);
                    if (kc == 0) { flag = VF_INSIDE; tlo = thi; slo = shi; }
                    else { flag = VF_BRACKET; tlo = j > 0 ? tb : prev_t; slo = j > 0 ? sb : prev_s; }
                    break;
                }
                prev_t = __shfl(t, 31, 64);
                prev_s = __shfl(sdf, 31, 64);
            }
        }
        if (lane == 0) {
            float4 *b = reinterpret_cast<float4 *>(v.brk + (size_t)ray * VBRK);
            b[0] = make_float4(tlo, thi, slo, shi);
            b[1] = make_float4(__int_as_float(flag), __int_as_float(kc), __int_as_float(tiles), 0.f);
        }
    }
}

template <typename TM, typename TT>
__global__ __launch_bounds__(256) void k_view_shade(FieldArgs a, ViewArgs v) {
    constexpr bool HALF = sizeof(TM) == 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    TM *s_fr = reinterpret_cast<TM *>(smem);
    float *s_b = staged_bias<TM, N_FRAGS>(smem);
    // amp: the colour pass's bias image rounded to fp16, as in k_query_field
    NOF_STAGE_FRAGS(TM, N_FRAGS, 0, HALF, a, smem, s_b);
    __syncthreads();
    const int lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const LdsW<TM> W{s_fr};
    const float *s_bc = HALF ? s_b + BIAS_WORDS : s_b;
    const int ntile = (v.n + 31) / 32;
    for (int tl = (int)blockIdx.x * 4 + wave; tl < ntile; tl += (int)gridDim.x * 4) {
        const int idx = tl * 32 + n;
        const bool inb = idx < v.n;
        float d[3] = {0.f, 0.f, 0.f}, vz = 0.f, lo = 0.f, hi = 0.f, slo = 0.f, shi = 0.f;
        int flag = VF_MISS, kc = -1, tiles = 0;
        if (inb) {
            const float4 r0 = reinterpret_cast<const float4 *>(v.vray + (size_t)idx * VRAY)[0];
            const float4 *b = reinterpret_cast<const float4 *>(v.brk + (size_t)idx * VBRK);
            const float4 b0 = b[0], b1 = b[1];
            d[0] = r0.x; d[1] = r0.y; d[2] = r0.z; vz = r0.w;
            lo = b0.x; hi = b0.y; slo = b0.z; shi = b0.w;
            flag = __float_as_int(b1.x); kc = __float_as_int(b1.y); tiles = __float_as_int(b1.z);
        }
        const bool hit = flag != VF_MISS, ref = flag == VF_BRACKET;
        float ts = lo, g[3] = {0.f, 0.f, 0.f}, rgb[3] = {0.f, 0.f, 0.f};
        if (__any(hit)) {
            if (__any(ref)) {
                for (int it = 0; it < v.n_refine; ++it) {
                    const float mid = 0.5f * (lo + hi);
                    float x[3];
                    view_point(v, d, mid, x);
                    const float s = tile_sdf<TM, TT>(a, W, s_b, x, ref, lane);
                    if (ref) {
                        if (s > 0.f) { lo = mid; slo = s; }
                        else { hi = mid; shi = s; }
                    }
                }
            }
            if (ref) ts = lo + ((hi - lo) * slo) / (slo - shi);
            float x[3], sdf, r[3] = {0.f, 0.f, 0.f}, logit[3] = {0.f, 0.f, 0.f};
            view_point(v, d, ts, x);
            query_tile<TM, TT, true>(a, W, s_b, s_bc, x, hit, true, true, true, v.ff, v.n_ff, d, lane, sdf, r, logit);
            if (hit) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    g[c] = 0.5f * r[c];   // query_field's gradient
                    rgb[c] = 1.f / (1.f + expf(-logit[c]));
                }
                const float gn = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
#pragma unroll
                for (int c = 0; c < 3; ++c) g[c] = gn > 0.f ? g[c] / gn : 0.f;
            }
        }
        if (inb && h == 0) {
            v.t[idx] = hit ? ts : 0.f;
            v.depth[idx] = hit ? ts * vz : 0.f;
            v.hit[idx] = hit ? 1 : 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                v.normal[(size_t)idx * 3 + c] = g[c];
                v.rgb[(size_t)idx * 3 + c] = rgb[c];
            }
            if (v.index) v.index[idx] = kc;
            if (v.tiles) v.tiles[idx] = tiles;
        }
    }
}

}  // namespace nof
