// Forward-only ray render (nof_render_rays): what NerfRunner.render_images needs of render_rays
// (nerf_runner.py:1043-1087), raw2outputs (:1131-1168) and the depth rule of render_images (:602-610),
// without anything of the training step: no tile records for a backward, no feature stores, no flags,
// no losses, no atomics. It uses the device functions the step uses, from field_core.h — sample_z,
// sample_point, encode_levels, mlp_sdf_net, mlp_colour_net, bell_weight — as they are.
//
//  * k_render_ctx: a thread per ray — the per-ray context record (store_ray_ctx) in the render's
//    own workspace.
//  * k_render: persistent 8-wave blocks, a wave per (ray, 32-sample tile): unperturbed z, validity,
//    the multires encode from the pair table (tiles with no sample inside the box skip the gathers and
//    run the sigma net on the zero encoding, as run_network :1246,1265 leaves it), the sigma net, and —
//    only where some valid sample has a non-zero weight — the colour net. Per tile one 48-B record:
//    the weight sum and composited colour (the same half-wave sums as k_encode / k_colour), and what
//    the zero-crossing rule needs across the tile's borders.
//  * k_render_final: a thread per ray walks its tiles in order (fixed order: two renders of the same
//    rays are bit-identical): rgb = sum / (weight sum + 1e-10), depth by the rule of :602-610.
//
// HBM traffic per ray at S = 192, L = 16, amp: the 128-B context record written and read by 6 tiles
// (scalar loads), <= 6 x 32 x 16 levels x 4 corner-pair loads of 8 B (98 KB, L2 / Infinity Cache
// hits for neighbouring samples), 6 records of 48 B written and read, 16 B of outputs; with the
// per-sample outputs 9 B per sample more. FLOPs per ray: sigma net 2 x (32 x 64 + 64 x 16) = 6.1 K per
// sample, colour net 2 x (32 x 64 + 64 x 64 + 64 x 16) = 14.3 K per sample of a colour tile (the K and
// M paddings of the MFMA tiles included): 1.2 M (sigma, 192 samples) + 0.46 M per colour tile.
#pragma once
#include "field_core.h"
#pragma clang fp contract(off)

namespace nof {

struct RenderOut {
    float *rgb;        // [R,3]
    float *depth;      // [R]
    float *z;          // [R,S] or null
    float *sdf;        // [R,S] or null
    uint8_t *valid;    // [R,S] or null
    float *rrec;       // [R*S/32][RREC] per-tile records (workspace)
};

// per tile: weight sum, composited colour | sdf and z of the tile's first and last sample | z of the
// first in-tile pair with a negative product, flag bits
constexpr int RREC = 12;
enum { RF_NONPOS = 1, RF_NEG = 2 };   // some in-tile product is not > 0 / is < 0

// fragments FR_L1 .. FR_B5 - 1 (the forward's 24 of the 46) and the bias image, staged once per block;
// behind them the waves' level tables (16 levels x 32 B each)
constexpr int RENDER_NFR = FR_B5, RENDER_WPB = 8;
constexpr size_t RENDER_LVT_BYTES = RENDER_WPB * 16 * 32;

__global__ __launch_bounds__(256) void k_render_ctx(FieldArgs a) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < a.R) store_ray_ctx(a.rctx, r, build_ray(a, r));
}

template <typename TM, typename TT>
__global__ __launch_bounds__(RENDER_WPB * 64) void k_render(FieldArgs a, RenderOut o) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const TM *s_fr = reinterpret_cast<const TM *>(smem);
    float *s_b = staged_bias<TM, RENDER_NFR>(smem);
    NOF_STAGE_FRAGS(TM, RENDER_NFR, 0, false, a, smem, s_b);
    const int lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint4 *lvt = reinterpret_cast<uint4 *>(smem + staged_bytes<TM, RENDER_NFR>()) + wave * 32;
    level_table(a, lvt, lane);
    __syncthreads();
    const int ntiles = a.S / 32;
    const int n_all = a.R * ntiles;   // nof_render_rays keeps R * S / 32 below 2^31
    LdsWt<TM> W(s_fr, lane);
    for (int gw = (int)blockIdx.x * RENDER_WPB + wave; gw < n_all; gw += (int)gridDim.x * RENDER_WPB) {
        const int r = gw / ntiles, t = gw - r * ntiles;
        const RayCtx c = load_ray<true>(a, r);
        const int s = 32 * t + n;
        const float z = sample_z(a, r, s, c.depth, c.vdepth, c.total, c.box);
        float p[3], x[3];
        const bool valid = sample_point(c, z, p, x);
        const float x01[3] = {(x[0] + 1) / 2, (x[1] + 1) / 2, (x[2] + 1) / 2};
        Acts<TM> A;
        frag_zero<TM>(A.X[0]);
        frag_zero<TM>(A.X[1]);
        if (__any(valid)) {
#pragma unroll
            for (int g0 = 0; g0 < 8; g0 += 2) {
                const int lvs[2] = {lane_level(g0 >> 2, g0 & 3, h), lane_level((g0 + 1) >> 2, (g0 + 1) & 3, h)};
                float v[2][2];
                encode_levels<TT, 2, true, true>(a, lvs, valid, x01, v, lvt);
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    frag_set<TM>(A.X[(g0 + k) >> 2], 2 * ((g0 + k) & 3), v[k][0]);
                    frag_set<TM>(A.X[(g0 + k) >> 2], 2 * ((g0 + k) & 3) + 1, v[k][1]);
                }
            }
        }
        W.fence();   // the fragment reads stay in this tile
        float sdf;
        f16v l2;
        mlp_sdf_net<TM>(W, s_b, A, lane, sdf, l2);
        const float w = bell_weight(a, c.depth, z);
        const float wc = valid && w > 0.f ? w : 0.f;
        float rc[3] = {0.f, 0.f, 0.f};
        if (__any(wc > 0.f)) {
            const typename FragT<TM>::T shf = sh_frag<TM>(c, h, a.n_ff);
            float logit[3];
            uint32_t m3 = 0, m4 = 0;   // the ReLU masks are the backward's: not taken
            mlp_colour_net<TM>(W, s_b, A, l2, shf, lane, logit, false, m3, m4);
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) rc[cc] = wc * sigmoidf(logit[cc]);
        }
        // the tile's sums exactly as the training forward takes them (k_encode: the weight of every
        // sample in the lower half; k_colour: r | g, then b)
        float ws, s0, s1, s2, unused;
        half_sums(h == 0 ? w : 0.f, ws, unused);
        half_sums(h == 0 ? rc[0] : rc[1], s0, s1);
        half_sums(h == 0 ? rc[2] : 0.f, s2, unused);
        // zero-crossing rule inside the tile: pair (n, n + 1), n < 31; the pair across the tile's
        // border is k_render_final's. Both lane halves hold the same 32 samples.
        const float nxt = __shfl(sdf, (n + 1) & 31, 64);
        const float prod = nxt * sdf;
        const uint32_t neg = (uint32_t)__ballot(n < 31 && prod < 0.f);
        const uint32_t nonpos = (uint32_t)__ballot(n < 31 && !(prod > 0.f));
        const float z_neg = __shfl(z, neg ? __builtin_ctz(neg) : 0, 64);
        const float sdf_last = __shfl(sdf, 31, 64), z_last = __shfl(z, 31, 64);
        const float sdf_first = __shfl(sdf, 0, 64), z_first = __shfl(z, 0, 64);
        const int flags = (nonpos ? RF_NONPOS : 0) | (neg ? RF_NEG : 0);
        float4 *rec = reinterpret_cast<float4 *>(o.rrec + (size_t)gw * RREC);
        if (lane == 0) {
            rec[0] = make_float4(ws, s0, s1, s2);
            rec[1] = make_float4(sdf_first, sdf_last, z_first, z_last);
            rec[2] = make_float4(z_neg, __int_as_float(flags), 0.f, 0.f);
        }
        if (h == 0) {
            const size_t sid = (size_t)r * a.S + s;
            if (o.z) o.z[sid] = z;
            if (o.sdf) o.sdf[sid] = sdf;
            if (o.valid) o.valid[sid] = valid;
        }
    }
}

__global__ __launch_bounds__(256) void k_render_final(FieldArgs a, RenderOut o) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.R) return;
    const int ntiles = a.S / 32;
    float wtot = 0.f, racc[3] = {0.f, 0.f, 0.f};
    bool all_pos = true, found = false;
    float zj = 0.f, sdf_prev = 0.f, z_prev = 0.f;
    for (int t = 0; t < ntiles; ++t) {
        const float4 *q = reinterpret_cast<const float4 *>(o.rrec + ((size_t)r * ntiles + t) * RREC);
        const float4 q0 = q[0], q1 = q[1], q2 = q[2];
        wtot += q0.x; racc[0] += q0.y; racc[1] += q0.z; racc[2] += q0.w;
        if (t == 0) {
            zj = q1.z;   // no negative product anywhere: argmax of an all-false mask is 0
        } else {         // the pair across the border: signs[32 t - 1] = sdf[32 t] * sdf[32 t - 1]
            const float prod = q1.x * sdf_prev;
            all_pos = all_pos && prod > 0.f;
            if (prod < 0.f && !found) { found = true; zj = z_prev; }
        }
        const int flags = __float_as_int(q2.y);
        all_pos = all_pos && !(flags & RF_NONPOS);
        if ((flags & RF_NEG) && !found) { found = true; zj = q2.x; }
        sdf_prev = q1.y;
        z_prev = q1.w;
    }
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) o.rgb[(size_t)r * 3 + cc] = racc[cc] / (wtot + 1e-10f);
    o.depth[r] = all_pos ? a.far_sc : zj;
}

}  // namespace nof
