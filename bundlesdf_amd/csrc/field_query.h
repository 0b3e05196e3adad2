// Field point query (nof_query_field): SDF, its gradient with respect to the point, and the colour
// of the field at a list of points — the query side of NerfRunner: run_network_density(get_normals=
// True) (nerf_runner.py:1306-1346) and run_network as mesh_vertex_color_from_network calls it
// (:1411-1428, :1226-1303). With it, above it, the SDF query it grew from (nof_query_sdf: k_query_sdf),
// whose shape k_query_field keeps — one wave per tile of 32 points, the levels split over the
// two lane halves by lane_level, all 46 weight fragments and the bias image staged in LDS, a
// grid-stride loop over tiles. Both use field_core.h's device functions (gather_level, mlp_sdf_net,
// mlp_colour_net, the fragment helpers) as they are. No atomics; nothing is written but the
// requested output arrays.
//
// Per tile:
//  * forward: clip to [-1, 1], multires encode, sigma net, in k_query_sdf's instruction order: the
//    SDF is bit-identical to nof_query_sdf's on the same points.
//  * gradient (grad != null): while a level's corners are in registers its d feature / d x01 is
//    formed too (2 x 3 values: the trilinear sum with one axis' weight replaced by +-scale, the
//    reference's dy_dx, gridencoder.cu:202-245). A one-hot on the SDF row goes back through the sigma
//    net on MFMA (FR_B2: row 0 of sigma_net.2.weight, masked by the layer-1 ReLU; FR_B1: times
//    sigma_net.0.weight, the fragments the training backward reads), which leaves d sdf / d feature
//    of exactly the levels the lane encoded in its accumulator rows. The contraction with dy_dx runs
//    in the reference's order (kernel_input_backward :339-365: levels ascending, channels inside):
//    the running sums hop between the lane halves every two levels. Times 0.5 for x01 = (x + 1) / 2.
//    The gradient is with respect to the CLIPPED point (the reference makes the clipped tensor the
//    autograd leaf): a point outside the box gets the gradient at its clipped position, not zero.
//    amp rounds where the reference's autograd rounds: dy_dx to fp16 term by term (grid_oracle.c half
//    mode), both Linear input gradients to fp16, the input-backward products and running sums to fp16.
//  * colour (rgb != null): the colour net on [geo, sh3(0), frame features of one frame] and a
//    sigmoid. Validity here is run_network's, NOT run_network_density's: a point with any |x| > 1 is
//    not clipped — its grid embedding is zero and the nets still run (:1244-1265). So in one call a
//    point outside the box reads the SDF and gradient of its clipped position and the colour of a zero
//    embedding; tiles holding such a point run the sigma net a second time on the zeroed columns
//    (MFMA columns are independent: the other points' values do not change).
//    amp: the colour pass follows the autocast composition to the bit, which the project's forward
//    (k_query_sdf, k_render, the training step) does not: those round a feature to fp16 once after
//    its fp32 sum and add the fp32 bias, the reference's half kernel rounds every term
//    (gridencoder.cu:171-195 in half) and autocast casts the bias to fp16. One fp16 ulp of a colour
//    logit is more than the reference's own amp-vs-fp32 distance, so the colour pass takes its own
//    features (the same corner reads, summed as the half kernel sums them) through both nets with the
//    bias image rounded to fp16; the SDF keeps nof_query_sdf's bits.
#pragma once
#include "field_core.h"
#pragma clang fp contract(off)

namespace nof {

// ------------------------------------------- SDF query (mesh extraction)
// run_network_density (nerf_runner.py:1306-1346) on a dense grid or a point
// list: clip to [-1,1], multires encode, sigma net (L1, ReLU, L2) -> sdf.
// Grid mode follows extract_mesh (:1349-1382): point (i,j,k) = (gx[i], gy[j],
// gz[k]) in meshgrid 'ij' order; points whose octree voxel at the ray-tracing
// level is empty are not queried and read 1.0. One wave per 32 points; the
// encode is spread over both lane halves exactly as in k_encode and the MLP
// runs on MFMA with the weights staged in LDS.
struct QueryArgs {
    const float *pts;                  // [n,3] (point mode) or null
    const float *gx, *gy, *gz;         // grid axes (grid mode)
    int nx, ny, nz;
    int64_t n;
    const uint8_t *occ;                // [N^3] occupancy at the ray-tracing level (x fastest) or null
    int occ_n;
    float *sdf;                        // [n]
};

template <typename TM, typename TT>
__global__ __launch_bounds__(256) void k_query_sdf(FieldArgs a, QueryArgs q) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    TM *s_fr = reinterpret_cast<TM *>(smem);
    float *s_b = staged_bias<TM, N_FRAGS>(smem);
    NOF_STAGE_FRAGS(TM, N_FRAGS, 0, false, a, smem, s_b);
    __syncthreads();
    const int lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t ntile = (q.n + 31) / 32;
    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < ntile; t += (int64_t)gridDim.x * 4) {
        const int64_t idx = t * 32 + n;
        const bool inb = idx < q.n;
        float x[3] = {0.f, 0.f, 0.f};
        if (inb) {
            if (q.pts) {
#pragma unroll
                for (int d = 0; d < 3; ++d) x[d] = q.pts[idx * 3 + d];
            } else {
                const int64_t k = idx % q.nz, ij = idx / q.nz;
                const int64_t j = ij % q.ny, i = ij / q.ny;
                x[0] = q.gx[i]; x[1] = q.gy[j]; x[2] = q.gz[k];
            }
        }
        bool valid = inb;
        if (inb && q.occ) {   // OctreeManager.get_center_ids >= 0 (Utils.py:392-394)
            const float N = (float)q.occ_n;
            uint32_t c[3];
            bool inside = true;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                inside = inside && fabsf(x[d]) <= 1.f;
                const float f = floorf((x[d] + 1.f) * 0.5f * N);
                c[d] = (uint32_t)fminf(fmaxf(f, 0.f), N - 1.f);
            }
            valid = inside && q.occ[((size_t)c[2] * q.occ_n + c[1]) * q.occ_n + c[0]] != 0;
        }
        if (!__any(valid)) {
            if (inb && h == 0) q.sdf[idx] = 1.f;
            continue;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) x[d] = fminf(fmaxf(x[d], -1.f), 1.f);   // torch.clip(inputs, -1, 1)
        const float x01[3] = {(x[0] + 1) / 2, (x[1] + 1) / 2, (x[2] + 1) / 2};
        Acts<TM> A;
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                const int lv = lane_level(ss, qq, h);
                float v[2] = {0.f, 0.f};
                if (inb && lv < (int)a.L) encode_level<TT>(a, level_info(a, lv), x01, v);
                frag_set<TM>(A.X[ss], 2 * qq, v[0]);
                frag_set<TM>(A.X[ss], 2 * qq + 1, v[1]);
            }
        }
        float sdf;
        f16v l2;
        mlp_sdf_net<TM>(LdsW<TM>{s_fr}, s_b, A, lane, sdf, l2);
        if (inb && h == 0) q.sdf[idx] = valid ? sdf : 1.f;
    }
}

struct QueryFieldArgs {
    const float *pts;      // [n,3]
    int64_t n;
    const float *ff;       // the frame's feature row (n_ff floats) or null
    int n_ff;
    float *sdf;            // [n] or null
    float *grad;           // [n,3] or null
    float *rgb;            // [n,3] or null
};

// encode_level (the same sums in the same order: the same feature bits) and, when `dx`, the level's
// d feature / d x01 [axis][channel]; fh (amp, when `hm`): the feature as the reference's half kernel
// sums it, every product and every partial sum rounded to fp16
template <typename TT>
__device__ __forceinline__ void encode_level_dx(const FieldArgs &a, const LevelInfo &li, const float x01[3], float f[2],
                                                bool dx, float dydx[3][2], bool hm, float fh[2]) {
    constexpr bool HALF = sizeof(TT) == 2;
    float pos[3], e[8][2];
    uint32_t rows[8];
    gather_level<TT, true>(a, li, x01, pos, e, rows);
    f[0] = 0.f; f[1] = 0.f;
#pragma unroll
    for (int idx = 0; idx < 8; ++idx) {
        float w = 1.f;
#pragma unroll
        for (int d = 0; d < 3; ++d) w *= ((idx >> d) & 1) ? pos[d] : 1 - pos[d];
        f[0] = __builtin_fmaf(w, e[idx][0], f[0]);
        f[1] = __builtin_fmaf(w, e[idx][1], f[1]);
        if constexpr (HALF) {
            if (hm) {
                fh[0] = round_h(fh[0] + round_h(w * e[idx][0]));
                fh[1] = round_h(fh[1] + round_h(w * e[idx][1]));
            }
        }
    }
    if (!dx) return;
#pragma unroll
    for (int gd = 0; gd < 3; ++gd) {
        float rg[2] = {0.f, 0.f};
#pragma unroll
        for (int idx = 0; idx < 4; ++idx) {
            float w = li.scale;
            int c = 0;   // the corner with axis gd's bit clear
#pragma unroll
            for (int nd = 0; nd < 2; ++nd) {
                const int d = nd >= gd ? nd + 1 : nd, bit = (idx >> nd) & 1;
                w *= bit ? pos[d] : 1 - pos[d];
                c |= bit << d;
            }
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                const float diff = e[c | (1 << gd)][ch] - e[c][ch];
                if constexpr (HALF) rg[ch] = round_h(rg[ch] + round_h(w * round_h(diff)));
                else rg[ch] = __builtin_fmaf(w, diff, rg[ch]);
            }
        }
        dydx[gd][0] = rg[0];
        dydx[gd][1] = rg[1];
    }
}

// One tile of 32 points (lane n and n + 32 hold point n): the forward, the gradient and the colour pass
// described above, as k_query_field runs them; the surface render's shading kernel (field_view.h) runs
// the same tile at its hit points. x: the point as given (not clipped); sdf is returned on every lane,
// r (d sdf / d x01 summed over the levels: the gradient is 0.5 r) and logit on the lanes of half 0.
// VIEW: the colour net's SH input is sh3(vdir) as sh_frag lays it out, else sh3(0) (the constant term).
template <typename TM, typename TT, bool VIEW>
__device__ __forceinline__ void query_tile(const FieldArgs &a, const LdsW<TM> &W, const float *s_b, const float *s_bc,
                                           float x[3], bool inb, bool want_sdf, bool want_dx, bool want_rgb,
                                           const float *ff, int n_ff, const float vdir[3], int lane, float &sdf,
                                           float r[3], float logit[3]) {
    typedef typename FragT<TM>::T Frag;
    constexpr bool HALF = sizeof(TM) == 2;
    const int h = lane >> 5;
    // run_network's validity (:1244); the SDF and the gradient take the clipped point instead
    const bool inside = fabsf(x[0]) <= 1.f && fabsf(x[1]) <= 1.f && fabsf(x[2]) <= 1.f;
#pragma unroll
    for (int d = 0; d < 3; ++d) x[d] = fminf(fmaxf(x[d], -1.f), 1.f);   // torch.clip(inputs, -1, 1)
    const float x01[3] = {(x[0] + 1) / 2, (x[1] + 1) / 2, (x[2] + 1) / 2};
    // colour alone: the zero embedding of a point outside the box needs no gather
    const bool enc = inb && (want_sdf || inside);
    Acts<TM> A;
    Frag Xc[2];            // amp: the colour pass's features (half-kernel rounding)
    float dydx[8][3][2];   // this lane's 8 levels (k = 4 ss + qq)
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int lv = lane_level(ss, qq, h), k = 4 * ss + qq;
            float v[2] = {0.f, 0.f}, vh[2] = {0.f, 0.f};
#pragma unroll
            for (int d = 0; d < 3; ++d) { dydx[k][d][0] = 0.f; dydx[k][d][1] = 0.f; }
            if (enc && lv < (int)a.L)
                encode_level_dx<TT>(a, level_info(a, lv), x01, v, want_dx, dydx[k], want_rgb && inside, vh);
            frag_set<TM>(A.X[ss], 2 * qq, v[0]);
            frag_set<TM>(A.X[ss], 2 * qq + 1, v[1]);
            if constexpr (HALF) {
                frag_set<TM>(Xc[ss], 2 * qq, vh[0]);
                frag_set<TM>(Xc[ss], 2 * qq + 1, vh[1]);
            }
        }
    }
    sdf = 0.f;
    f16v l2;
    if (want_sdf) mlp_sdf_net<TM>(W, s_b, A, lane, sdf, l2);

    if (want_dx) {
        // one-hot on the SDF row (row 0 = element 0 of lane half 0) back through L2 and the ReLU
        Frag dH2;
        frag_zero<TM>(dH2);
        if (h == 0) frag_set<TM>(dH2, 0, 1.f);
        f16v acc[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            acc_zero(acc[mt]);
            mma(acc[mt], W.get(FR_B2 + mt * 2, lane), dH2);
        }
        Frag dH1[2][2];
        masked_frags<TM>(acc, relu_mask<TM>(A.H1), dH1);
        // d sdf / d feature = B1 dH1, in this lane's level order (register 8 ss + 2 qq + channel)
        acc_zero(acc[0]);
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) mma(acc[0], W.get(FR_B1 + 2 * t2 + s2, lane), dH1[t2][s2]);
        // kernel_input_backward's sum, levels ascending: levels 2 m, 2 m + 1 live in lane half
        // m & 1 (lane_level), so the running sums change halves after every pair of levels
        r[0] = 0.f; r[1] = 0.f; r[2] = 0.f;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int ss = m >> 2, qb = 2 * ((m >> 1) & 1), hh = m & 1;
            float rn[3] = {r[0], r[1], r[2]};
#pragma unroll
            for (int qi = 0; qi < 2; ++qi) {
                const int qq = qb + qi, k = 4 * ss + qq;
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) {
                    float g = acc[0][8 * ss + 2 * qq + ch];
                    if constexpr (HALF) g = round_h(g);   // the fp16 Linear input gradient
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        if constexpr (HALF) rn[d] = round_h(rn[d] + round_h(g * dydx[k][d][ch]));
                        else rn[d] = __builtin_fmaf(g, dydx[k][d][ch], rn[d]);
                    }
                }
            }
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float other = __shfl_xor(rn[d], 32, 64);
                r[d] = h == hh ? rn[d] : other;
            }
        }
    }

    if (want_rgb) {
        // the colour pass's sigma net: fp32 reuses the SDF's unless the tile holds a point outside the box
        if (HALF || !want_sdf || __any(inb && !inside)) {
            if constexpr (HALF) {
                A.X[0] = Xc[0];   // zero where !inside (never encoded)
                A.X[1] = Xc[1];
            } else if (!inside) {
                frag_zero<TM>(A.X[0]);
                frag_zero<TM>(A.X[1]);
            }
            float unused;
            mlp_sdf_net<TM>(W, s_bc, A, lane, unused, l2);
        }
        // sh3 of the view direction ((0, 0, 0): only the constant term) and the frame's features, as
        // sh_frag places them
        Frag shf;
        frag_zero<TM>(shf);
        if constexpr (VIEW) {
            const float vx = vdir[0], vy = vdir[1], vz = vdir[2];
            const float xx = vx * vx, yy = vy * vy, zz = vz * vz;
            if (h == 0) {
                frag_set<TM>(shf, 0, SH_C0);
                frag_set<TM>(shf, 1, -SH_C1 * vy);
                frag_set<TM>(shf, 2, SH_C1 * vz);
                frag_set<TM>(shf, 3, -SH_C1 * vx);
                frag_set<TM>(shf, 4, SH_C2_4 * (xx - yy));
            } else {
                frag_set<TM>(shf, 0, SH_C2_0 * (vx * vy));
                frag_set<TM>(shf, 1, SH_C2_1 * (vy * vz));
                frag_set<TM>(shf, 2, SH_C2_2 * ((2.0f * zz - xx) - yy));
                frag_set<TM>(shf, 3, SH_C2_3 * (vx * vz));
            }
        } else if (h == 0) {
            frag_set<TM>(shf, 0, SH_C0);
        }
        if (h == 0 && ff) {
#pragma unroll
            for (int j = 0; j < 3; ++j) frag_set<TM>(shf, 5 + j, j < n_ff ? ff[j] : 0.f);
        }
        uint32_t m3 = 0, m4 = 0;
        mlp_colour_net<TM>(W, s_bc, A, l2, shf, lane, logit, false, m3, m4);
    }
}

template <typename TM, typename TT>
__global__ __launch_bounds__(256) void k_query_field(FieldArgs a, QueryFieldArgs q) {
    constexpr bool HALF = sizeof(TM) == 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    TM *s_fr = reinterpret_cast<TM *>(smem);
    float *s_b = staged_bias<TM, N_FRAGS>(smem);
    // amp: a second bias image rounded to fp16 (autocast's bias) for the colour pass
    NOF_STAGE_FRAGS(TM, N_FRAGS, 0, HALF, a, smem, s_b);
    __syncthreads();
    const int lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const LdsW<TM> W{s_fr};
    const float *s_bc = HALF ? s_b + BIAS_WORDS : s_b;   // the colour pass's bias image
    const bool want_dx = q.grad != nullptr, want_sdf = q.sdf != nullptr || want_dx, want_rgb = q.rgb != nullptr;
    const int64_t ntile = (q.n + 31) / 32;
    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < ntile; t += (int64_t)gridDim.x * 4) {
        const int64_t idx = t * 32 + n;
        const bool inb = idx < q.n;
        float x[3] = {0.f, 0.f, 0.f};
        if (inb) {
#pragma unroll
            for (int d = 0; d < 3; ++d) x[d] = q.pts[idx * 3 + d];
        }
        float sdf, r[3], logit[3];
        query_tile<TM, TT, false>(a, W, s_b, s_bc, x, inb, want_sdf, want_dx, want_rgb, q.ff, q.n_ff, nullptr, lane,
                                  sdf, r, logit);
        if (inb && h == 0) {
            if (q.sdf) q.sdf[idx] = sdf;
            if (want_dx) {
#pragma unroll
                for (int d = 0; d < 3; ++d) q.grad[idx * 3 + d] = 0.5f * r[d];   // x01 = (x + 1) / 2
            }
            if (want_rgb) {
#pragma unroll
                for (int c = 0; c < 3; ++c) q.rgb[idx * 3 + c] = 1.f / (1.f + expf(-logit[c]));
            }
        }
    }
}

}  // namespace nof
