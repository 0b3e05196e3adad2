// The device core the training step (field_step.hip) and the inference side (field_infer.hip) share:
// FieldArgs, the MFMA fragment (on mfma_tile.h) and wave helpers, the sampler, the forward encode, the MLP forward, the
// ray context, the SH input, the LDS staging of weight fragments. Device functions only, no kernel.
#pragma once
#include <type_traits>

#include "mfma_tile.h"
#include "ray_trace.h"
#include "mlp_lds.h"

// contraction off from here on (the headers above keep the default); every includer repeats the pragma
#pragma clang fp contract(off)
// Timing-only ablation switches (scripts/ablate.py) exist only in a build with
// -DNOF_ABLATE=1; in the product library every ABL() test is a compile-time false.
#ifndef NOF_ABLATE
#define NOF_ABLATE 0
#endif
#define ABL(bits) (NOF_ABLATE && (a.ablate & (bits)))
#define ABL_HOST(d, bits) (NOF_ABLATE && ((d)->ablate & (bits)))
// level quarter q (levels 4q .. 4q+3) skipped by the scatter (timing build)
#define ABL_SKIPQ(q) ((q) < 2 ? (1 << (23 + (q))) : (1 << (27 + (q))))

namespace nof {

constexpr int MLP_N_MAX = 9107 + 64 * 3;   // NeRFSmall(2x64, geo 15, colour 3x64), input <= 32, views 9 (+ <= 3 frame features)
// flat-parameter offsets (MLP_KEYS order, bundlesdf_amd/mlp_layout.py) for input width IN
struct MlpOff {
    int w1, b1, w2, b2, w3, b3, w4, b4, w5, b5, n, in, cin;
    // FF = frame_features: color_net.0 input = [frame features (FF), SH (9), geo (15)] (nerf_runner.py:221,1277)
    __host__ __device__ MlpOff(int IN, int FF = 0) : in(IN), cin(24 + FF) {
        w1 = 0; b1 = 64 * IN; w2 = b1 + 64; b2 = w2 + 16 * 64; w3 = b2 + 16; b3 = w3 + 64 * cin; w4 = b3 + 64;
        b4 = w4 + 64 * 64; w5 = b4 + 64; b5 = w5 + 3 * 64; n = b5 + 3;
    }
};
// fragment ids (bundlesdf_amd/mlp_layout.py)
constexpr int FR_L1 = 0, FR_L2 = 4, FR_L3 = 8, FR_L4 = 12, FR_L5 = 20, FR_B5 = 24, FR_B4 = 26, FR_B3 = 34,
              FR_B2 = 38, FR_B1 = 42, N_FRAGS = 46;
// Cin row k -> column of color_net.0.weight for ff frame features: rows 1..15 geo,
// 16..24 SH, 25..25+ff-1 the ray's frame features (mlp_layout.cin_to_w3_col).
__device__ __forceinline__ int cin_col(int i, int ff) {
    return (i >= 1 && i <= 15) ? ff + 9 + i - 1
                               : ((i >= 16 && i <= 24) ? ff + i - 16 : ((i >= 25 && i < 25 + ff) ? i - 25 : -1));
}
constexpr float SH_C0 = 0.28209479177387814f, SH_C1 = 0.4886025119029199f;
constexpr float SH_C2_0 = 1.0925484305920792f, SH_C2_1 = -1.0925484305920792f, SH_C2_2 = 0.31539156525252005f,
                SH_C2_3 = -1.0925484305920792f, SH_C2_4 = 0.5462742152960396f;

struct FieldArgs {
    const float *rays;        // [R,12] batch (dir3 rgb3 depth mask frame type near far)
    const float *tf;          // [F,16] world_from_cam (pose correction applied), row-major
    const float *intervals;   // [R,Kmax,2] z units
    const float *totals;      // [R]
    float *rctx;              // [R][RCTX] per-ray context records (k_ray_ctx, workspace)
    const float *t_rand;      // [R,S] or null (counter RNG)
    uint32_t seed;
    int R, Kmax, N_oct, N_dep, S;
    int perturb;
    float near_sc, far_sc, trunc, ntr, lambda, fs_sdf, ffw, rgb_w, fs_w, empty_w, trunc_w;
    float fs_rgb_w;           // cfg fs_rgb_weight: colour of front (free-space) samples pulled to white (train_loop :728-731)
    float inv_3R, inv_RS, inv_3RS;
    const float *loss_scale;  // device scalar (GradScaler scale; 1 in fp32 mode)
    const void *table;        // [T,2] (float or half)
    const float4 *levels;     // [L]: scale, res (bits), row offset (bits), rows (bits)
    uint32_t L;
    int mlp_in;               // L*C
    int n_ff;                 // frame_features (0..3): per-frame latent code fed to the colour net
    const float *ff;          // [F, n_ff] f32 (FeatureArray.data)
    float *grad_ff;           // [F, n_ff] f32 (scaled like grad_mlp)
    const void *frags;        // [46][64][8] TM
    const float *bias;        // [5][64]
    float *grad_table;        // [T,2] f32 (fp32 mode)
    __half *grad_table16;     // [T,2] f16 (amp mode: the reference's __half2 gradient, gridencoder.cu:319-327)
    float *grad_mlp;          // [9107] f32
    float *ray_grad;          // [R,12]
    uint32_t *tile_gmask;     // [R*S/32] k_encode -> k_scatter: bit n = sample n of the tile carries a loss gradient
    const uint4 *quads;       // amp, R >= 32 K: xy-quad mirror of the fp16 table (k_quad_mirror), or null
    uint32_t n_rows;          // table rows (the quad mirror's length)
    bool quads_ready;         // the caller rebuilt `quads` for this step (nof_quad_mirror on a side stream)
    float *loss_part;         // [LOSS_COPIES][16] per-wave loss / counter partials (workspace), folded into loss_acc
    float *loss_acc;          // [8 + 128 + 8]: rgb, fs, empty, sdf (normalised), n_valid, n_bwd, -, -; [8 + 2i + {0,1}] HBM scatter atomics (flush, direct), spread; [136..139] work counters
    float *dbg_z;             // [R,S]
    float *dbg_raw;           // [R,S,4]
    uint8_t *dbg_valid;       // [R,S]
    float *dbg_rgb;           // [R,3]
    void *feat;               // [R*S*32] TM features, fragment order (workspace)
    void *dfeat;              // [16][R*S][2] TM dL/dfeature (scaled), level-major (store_dfeat; workspace)
    float *zbuf;              // [R*S] sample z (workspace)
    uint8_t *tile_bwd;        // [R*S/32] tile ran the backward (workspace)
    uint32_t slot_mask;       // scatter LDS hash slots per wave - 1 (power of two)
    int *tile_sid;            // [R*S/32] list of flagged tiles: first sample id | sigma-only bit (k_compact; workspace)
    int *n_tiles;             // device counter of records (workspace)
    float *ray_aux;           // [R][RAY_AUX] k_ray_final -> k_mlp_bwd / k_scatter (workspace)
    float4 *tile_aux;         // [R*S/32][TILE_AUX] per-record masks + loss terms (workspace)
    int ablate;               // timing-only ablation bits (builds with -DNOF_ABLATE=1 only; results invalid otherwise)
    int xcd_order;            // bit 0: k_encode, bit 1: k_scatter blocks in XCD-contiguous order (xcd_block)
    const nof_step_params *sp;   // device step block (graph replay) or null: trunc / seed from it
    int no_dx;                // poses frozen: no input gradient (no corner re-gather, no dL/dtf)
    int scatter_lpw;          // k_scatter levels per wave (L: wave per ray; fewer: waves per (ray, level group))
    float *rrec;              // [R*S/32][TREC] per-tile partial sums (k_encode SIG / k_colour -> k_ray_final; workspace)
    int *ctile_list;          // [R*S/32] colour tiles (flag 1 or 3) as first sample id (k_compact; workspace)
    int bwd_flush;            // k_mlp_bwd_tr weight-gradient flush: 0 by batch size, 1 per wave, 2 block-reduced
    int count_atomics;        // the scatter kernels count their HBM atomics into loss_acc[8..135] (diagnostics)
    int compact_per;          // k_compact flags per block (0: by batch size; tests force the 16-flags-per-thread path)
    int encode_group;         // k_encode levels per lane with gathers in flight together (resolved: 1, 2 or 4)
};

// The kernels' view of the step's scalars: the device step block when given (one
// captured graph replays every step), else the values the host put in the descriptor.
__device__ __forceinline__ FieldArgs step_args(const FieldArgs &a0) {
    FieldArgs a = a0;
    if (a0.sp) {
        a.trunc = a0.sp->trunc;
        a.seed = a0.sp->seed;
    }
    return a;
}

// The field kernels' FieldArgs (their only kernel argument, at offset 0 of the kernarg segment)
// through a pointer the compiler cannot see through (laundered in the constant address space, so the
// reads stay scalar loads): the reads after it are issued there, not hoisted to the kernel's start
// and held in SGPRs across its gathers
__device__ __forceinline__ const FieldArgs &late_args() {
    auto k = __builtin_amdgcn_kernarg_segment_ptr();   // constant address space: scalar loads
    asm volatile("" : "+s"(k));
    return *(const FieldArgs *)k;
}

// ----------------------------------------------------------------- helpers
// Wave reductions on DPP (no LDS traffic): inclusive prefix sums inside each 16-lane
// row (row_shr 1, 2, 4, 8), then row_bcast:15 carries row totals into rows 1 / 3 and
// row_bcast:31 the first half's total into the second half. Must be called with the
// whole wave active (every call site is wave-uniform).
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROWS, 0xf, true));
}
__device__ __forceinline__ float row_prefix(float v) {
    v = dpp_add<0x111>(v);   // row_shr:1
    v = dpp_add<0x112>(v);   // row_shr:2
    v = dpp_add<0x114>(v);   // row_shr:4
    return dpp_add<0x118>(v);   // row_shr:8
}
__device__ __forceinline__ float lane_value(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
__device__ __forceinline__ float wave_sum(float v) {
    v = row_prefix(v);
    v = dpp_add<0x142, 0xa>(v);   // row_bcast:15 -> rows 1, 3
    v = dpp_add<0x143, 0xc>(v);   // row_bcast:31 -> rows 2, 3
    return lane_value(v, 63);
}
// sums of the two 32-lane halves, both returned wave-uniform
__device__ __forceinline__ void half_sums(float v, float &s0, float &s1) {
    v = row_prefix(v);
    v = dpp_add<0x142, 0xa>(v);
    s0 = lane_value(v, 31);
    s1 = lane_value(v, 63);
}

// v_rcp_f32 (1 ulp) instead of an IEEE division: ~10 instructions fewer per call
__device__ __forceinline__ float sigmoidf(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
// The dispatcher hands block b to XCD b % 8. xcd_block maps it to a logical
// block so each XCD (own 4 MB L2) works a contiguous range of blocks: with
// frame-major ray batches an XCD then gathers the table rows of ~2 views.
__device__ __forceinline__ int xcd_block(int b, int nb) {
    const int per = nb >> 3, rem = nb & 7, x = b & 7, i = b >> 3;
    return (x < rem ? x * (per + 1) : rem * (per + 1) + (x - rem) * per) + i;
}

__device__ __forceinline__ uint32_t hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float rng_uniform(uint32_t seed, uint32_t ray, uint32_t s) {
    uint32_t h = hash32(seed ^ hash32(ray * 0x9E3779B1U + hash32(s + 0x632BE5ABU)));
    return (float)(h >> 8) * (1.0f / 16777216.0f);
}

// torch.linspace(0, 1, n)[i] (two-sided FMA formula of ATen's range factory)
__device__ __forceinline__ float linspace01(int i, int n) {
    if (n == 1) return 0.0f;
    const float step = 1.0f / (float)(n - 1);
    return (i < n / 2) ? __builtin_fmaf(step, (float)i, 0.0f) : __builtin_fmaf(-step, (float)(n - 1 - i), 1.0f);
}

// Fragment types: 8 elements per lane per 16-wide K step.
template <typename TM> struct FragT;
template <> struct FragT<_Float16> { typedef h8v T; };
template <> struct FragT<float> { struct T { float v[8]; }; };

template <typename TM> __device__ __forceinline__ void frag_set(typename FragT<TM>::T &f, int j, float x);
template <> __device__ __forceinline__ void frag_set<_Float16>(h8v &f, int j, float x) { f[j] = (_Float16)x; }
template <> __device__ __forceinline__ void frag_set<float>(FragT<float>::T &f, int j, float x) { f.v[j] = x; }
template <typename TM> __device__ __forceinline__ float frag_get(const typename FragT<TM>::T &f, int j);
template <> __device__ __forceinline__ float frag_get<_Float16>(const h8v &f, int j) { return (float)f[j]; }
template <> __device__ __forceinline__ float frag_get<float>(const FragT<float>::T &f, int j) { return f.v[j]; }
template <typename TM> __device__ __forceinline__ void frag_zero(typename FragT<TM>::T &f) {
#pragma unroll
    for (int j = 0; j < 8; ++j) frag_set<TM>(f, j, 0.f);
}

// the float32 path of mma (fp16: mfma_tile.h)
__device__ __forceinline__ void mma(f16v &acc, const FragT<float>::T &a, const FragT<float>::T &b) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[j], b.v[j], acc, 0, 0, 0);
}

template <typename TM>
__device__ __forceinline__ typename FragT<TM>::T load_frag(const void *frags, int id, int lane) {
    typename FragT<TM>::T f;
    // Opaque per use: keeps the compiler from hoisting all 46 weight
    // fragments out of the ray loop into registers (that costs occupancy).
    asm volatile("" : "+s"(id));
    const TM *p = reinterpret_cast<const TM *>(frags) + ((size_t)id * 64 + lane) * 8;
    if constexpr (sizeof(TM) == 2) {
        f = *reinterpret_cast<const h8v *>(p);
    } else {
        const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
        f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w; f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
    }
    return f;
}

__device__ __forceinline__ void acc_init_bias(f16v &acc, const float *bias_row64, int mt, int h) {
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = bias_row64[32 * mt + acc_row(q, h)];
}
// fp16 pair helpers (packed instructions: one v_cvt_pk_f16_f32 / v_pk_max_f16 /
// v_and_b32 per two elements instead of per-element convert / max / select)
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ h2v pk_round(float a, float b) { return h2v{(_Float16)a, (_Float16)b}; }
__device__ __forceinline__ void frag_put2(h8v &f, int p, h2v u) { f[2 * p] = u[0]; f[2 * p + 1] = u[1]; }
// fp16 ReLU of a packed pair as a signed 16-bit max with 0: every negative half (sign bit set,
// -0 included) becomes +0, the others stay — max(u, 0) for every non-NaN u, and the result's sign
// bits are always clear (pair_bits relies on it)
__device__ __forceinline__ h2v relu_pk(h2v u) {
    uint32_t r;
    asm("v_pk_max_i16 %0, %1, 0" : "=v"(r) : "v"(__builtin_bit_cast(uint32_t, u)));
    return __builtin_bit_cast(h2v, r);
}
// fp16 ReLU masks are kept per pair: pair P's low half at bit P, its high half at bit
// P + 16 (so a pair's two 0/1 halves, from one v_pk_min_u16, enter with one shift-or).
// the pair's ReLU-derivative bits (u > 0 per half; u is a relu_pk output: +0 or positive)
__device__ __forceinline__ uint32_t pair_bits(h2v u, int P) {
    const uint32_t x = __builtin_bit_cast(uint32_t, u);
    uint32_t y;
    // one packed unsigned min per pair (written as asm: the compiler expands min(x, 1) into
    // per-half compares and selects)
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(y) : "v"(x), "s"(0x00010001u));
    return y << P;
}
constexpr uint32_t MASK_ALL = 0xffffffffu;
// the pair u with the halves whose mask bits (P, P + 16) are clear zeroed: the two bits moved to bits 0
// and 16 (a 0 / 1 factor per half) times the halves' bit patterns by one packed 16-bit integer multiply
// — three instructions where expanding the bits into 0xffff masks and and-ing took four
__device__ __forceinline__ h2v pk_keep(h2v u, uint32_t m, int P) {
    const uint32_t f = (m >> P) & 0x00010001u;
    uint32_t r;
    asm("v_pk_mul_lo_u16 %0, %1, %2" : "=v"(r) : "v"(__builtin_bit_cast(uint32_t, u)), "v"(f));
    return __builtin_bit_cast(h2v, r);
}

// acc registers 8s..8s+7 -> fragment of K step s (optionally ReLU; fp16: rounded, then
// max(., 0) on the packed pair, the same values as rounding max(v, 0))
template <typename TM>
__device__ __forceinline__ void acc_to_frag(const f16v &acc, int s, bool relu, typename FragT<TM>::T &f) {
    if constexpr (sizeof(TM) == 2) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            h2v u = pk_round(acc[8 * s + 2 * p], acc[8 * s + 2 * p + 1]);
            if (relu) u = relu_pk(u);
            frag_put2(f, p, u);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = acc[8 * s + j];
            frag_set<TM>(f, j, relu ? fmaxf(v, 0.f) : v);
        }
    }
}


// wave-uniform data read through the constant address space: scalar loads
typedef const __attribute__((address_space(4))) uint32_t *ConstU32;

// ------------------------------------------------------------- the sampler
// z of sample s of ray r (render_rays :1060-1080 / sample_rays_uniform :67-87
// / sampleRaysUniformOccupiedVoxels common.cu:40-105).
__device__ __forceinline__ float sample_z(const FieldArgs &a, int r, int s, float depth, bool vdepth, float total,
                                          const float *__restrict__ box) {
    int idx, n;
    float near, far;
    bool walk;
    if (s < a.N_oct) { idx = s; n = a.N_oct; near = 0.f; far = total; walk = true; }
    else {
        idx = s - a.N_oct; n = a.N_dep;
        if (vdepth) { near = depth - a.trunc; far = depth + a.trunc * a.ntr; walk = false; }
        else { near = 0.f; far = total; walk = true; }
    }
    auto zlin = [&](int i) {
        const float t = linspace01(i, n);
        return near * (1.f - t) + far * t;
    };
    float z = zlin(idx);
    if (a.perturb) {
        const float zc = z;
        const float lower = (idx == 0) ? zc : .5f * (zc + zlin(idx - 1));
        const float upper = (idx == n - 1) ? zc : .5f * (zlin(idx + 1) + zc);
        const float u = a.t_rand ? a.t_rand[(size_t)r * a.S + s] : rng_uniform(a.seed, (uint32_t)r, (uint32_t)s);
        z = lower + (upper - lower) * u;
        z = fminf(fmaxf(z, near), far);
    }
    // common.cu:40-105 walk (sequential subtraction; exact reference rounding), over the ray's
    // interval list in batches of WB intervals read by one scalar load (box is wave-uniform:
    // every caller passes its wave's ray): each lane runs the same per-interval steps as the
    // reference's loop — rem -= len until rem <= len — as selects on the batch's scalar registers,
    // and the wave leaves once every lane has its interval. (A loop of one dependent scalar load
    // per interval cost 0.28 ms of the headline encode.) Lanes that do not walk are done at once.
    if (!__any(walk)) return z;   // a tile of around-depth samples only
    const ConstU32 bq = (ConstU32)(size_t)box;
    if (__uint_as_float(bq[0]) == 0.f) return walk ? 0.f : z;
    const float eps = 1e-4f;
    float rem = z, res = z, prev_out = 0.f;
    bool done = !walk;
    const int Kmax = a.Kmax;
    constexpr int WB = 8;   // intervals per batch: one 64-B scalar load
    int i = 0;
    for (; i + WB <= Kmax; i += WB) {
        float b[2 * WB];
#pragma unroll
        for (int k = 0; k < 2 * WB; ++k) b[k] = __uint_as_float(bq[2 * i + k]);
#pragma unroll
        for (int j = 0; j < WB; ++j) {
            const float zin = b[2 * j], zout = b[2 * j + 1];
            if (zin == 0.f) return done ? res : ((rem <= eps && i + j >= 1) ? prev_out : 0.f);
            const float len = zout - zin;
            const bool hit = !done && rem <= len;
            res = hit ? zin + rem : res;
            rem = done || hit ? rem : rem - len;
            done = done || hit;
            prev_out = zout;
        }
        if (!__any(!done)) return res;
    }
    for (; i < Kmax; ++i) {   // the last Kmax mod WB intervals, one at a time
        const float zin = __uint_as_float(bq[2 * i]), zout = __uint_as_float(bq[2 * i + 1]);
        if (zin == 0.f) return done ? res : ((rem <= eps && i >= 1) ? prev_out : 0.f);
        const float len = zout - zin;
        const bool hit = !done && rem <= len;
        res = hit ? zin + rem : res;
        rem = done || hit ? rem : rem - len;
        done = done || hit;
        prev_out = zout;
    }
    return done ? res : (rem <= eps ? __uint_as_float(bq[(Kmax - 1) * 2 + 1]) : 0.f);
}

// raw2outputs sdf2weights numerator (nerf_runner.py:1151-1158)
__device__ __forceinline__ float bell_weight(const FieldArgs &a, float depth, float z) {
    if (depth > a.far_sc) return 0.f;
    const float u = (depth - z) / a.trunc;
    float w = sigmoidf(u * a.lambda) * sigmoidf(-u * a.lambda);
    const float dz = z - depth;
    const bool m = (dz <= a.trunc * a.ntr) && (dz >= -a.trunc);
    return m ? w : 0.f;
}

// --------------------------------------------------------------- encoding
// One level of kernel_grid (gridencoder.cu:106-246) for this lane's sample:
// features (C=2) and, when want_d, d feature / d x01 (3 x 2).
struct LevelInfo { float scale; uint32_t res, off, hs; };
__device__ __forceinline__ LevelInfo level_info(const FieldArgs &a, int lv) {
    const float4 v = a.levels[lv];
    return {v.x, __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
}
// the same record read through the constant address space (lv wave-uniform): a scalar load
__device__ __forceinline__ LevelInfo level_info_uniform(const FieldArgs &a, int lv) {
    const ConstU32 p = (ConstU32)(size_t)(a.levels + lv);
    return {__uint_as_float(p[0]), p[1], p[2], p[3]};
}

// The fp16 table as a buffer resource: corner-pair loads take a 32-bit byte offset (one shift)
// instead of a 64-bit address per load (the table is < 2 GB)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t table_rsrc(const void *table) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(table), (short)0, 0x7fffffff, 0x00020000);
}
typedef uint32_t u2v __attribute__((ext_vector_type(2)));
typedef uint32_t u4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint2 table_pair16(__amdgpu_buffer_rsrc_t rsrc, uint32_t row) {
    const u2v v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, row * 4u, 0, 0);
    return make_uint2(v.x, v.y);
}

// Dense-level test (res+1)^3 <= rows and the dense row index. _v: in full-rate 24-bit integer
// multiplies (v_mul_u32_u24; v_mul_lo_u32 / 64-bit multiplies issue at quarter rate): rs <=
// 1625 keeps rs^3 < 2^32, and every operand stays below 2^24
// (written as instructions: the compiler otherwise widens them back to v_mul_lo_u32). Per-lane
// level values (k_encode's lane halves); a wave-uniform level keeps scalar arithmetic.
__device__ __forceinline__ uint32_t mul24(uint32_t a, uint32_t b) {
    uint32_t d;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ uint32_t mad24(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t d;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ bool level_dense_v(uint32_t rs, uint32_t hs) {
    return rs <= 1625u && mul24(mul24(rs, rs), rs) <= hs;
}
__device__ __forceinline__ uint32_t dense_base_v(uint32_t off, const uint32_t pg[3], uint32_t rs) {
    return off + pg[0] + mul24(mad24(pg[2], rs, pg[1]), rs);
}
__device__ __forceinline__ bool level_dense(uint32_t rs, uint32_t hs) { return (uint64_t)rs * rs * rs <= hs; }

// Rows of the 8 corners of cell pg (bit d of idx = +1 along d), as
// get_grid_index (gridencoder.cu:65-83). Dense levels ((res+1)^3 <= rows:
// every level at config 2) need one index plus constant offsets; hashed
// levels use grid_row per corner.
__device__ __forceinline__ void corner_rows(const LevelInfo &li, const uint32_t pg[3], uint32_t rows[8]) {
    const uint32_t rs = li.res + 1;
    if (level_dense(rs, li.hs)) {
        // dense: rs^3 <= rows < 2^32, so rs <= 1625 and the 24-bit multiplies are exact
        const uint32_t base = dense_base_v(li.off, pg, rs), rs2 = rs * rs;
#pragma unroll
        for (int idx = 0; idx < 8; ++idx)
            rows[idx] = base + (idx & 1) + ((idx >> 1) & 1 ? rs : 0u) + ((idx >> 2) & 1 ? rs2 : 0u);
    } else {
#pragma unroll
        for (int idx = 0; idx < 8; ++idx) {
            uint32_t pl[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) pl[d] = pg[d] + ((idx >> d) & 1);
            rows[idx] = li.off + grid_row<3>(0, false, li.hs, li.res, pl);
        }
    }
}

// Corner values of one level for this lane's sample (kernel_grid index math).
template <typename TT, bool PAIRED = false>
__device__ __forceinline__ void gather_level(const FieldArgs &a, const LevelInfo &li, const float x01[3], float pos[3],
                                             float e[8][2], uint32_t rows[8]) {
    const TT *tab = reinterpret_cast<const TT *>(a.table);
    uint32_t pg[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        pos[d] = __builtin_fmaf(x01[d], li.scale, 0.5f);
        pg[d] = (uint32_t)floorf(pos[d]);
        pos[d] -= (float)pg[d];
    }
    corner_rows(li, pg, rows);
    const uint32_t rs = li.res + 1;
    if (PAIRED && level_dense(rs, li.hs)) {
        // dense level: corners idx and idx+1 (x, x+1) are adjacent rows -> one
        // 2-row load per pair (dword-aligned multi-dword global loads are legal)
#pragma unroll
        for (int idx = 0; idx < 8; idx += 2) {
            const TT *p = tab + (size_t)rows[idx] * 2;
            if constexpr (sizeof(TT) == 4) {
                typedef float f4a __attribute__((ext_vector_type(4), aligned(8)));
                const f4a v = *reinterpret_cast<const f4a *>(p);
                e[idx][0] = v.x; e[idx][1] = v.y; e[idx + 1][0] = v.z; e[idx + 1][1] = v.w;
            } else {
                uint2 v;
                __builtin_memcpy(&v, p, 8);
                const __half2 h0 = __builtin_bit_cast(__half2, v.x), h1 = __builtin_bit_cast(__half2, v.y);
                e[idx][0] = __low2float(h0); e[idx][1] = __high2float(h0);
                e[idx + 1][0] = __low2float(h1); e[idx + 1][1] = __high2float(h1);
            }
        }
    } else {
#pragma unroll
        for (int idx = 0; idx < 8; ++idx) {
            const TT *p = tab + (size_t)rows[idx] * 2;
            if constexpr (sizeof(TT) == 4) {
                const float2 v = *reinterpret_cast<const float2 *>(p);
                e[idx][0] = v.x; e[idx][1] = v.y;
            } else {
                const __half2 v = *reinterpret_cast<const __half2 *>(p);
                e[idx][0] = __low2float(v); e[idx][1] = __high2float(v);
            }
        }
    }
}

template <typename TT>
__device__ __forceinline__ void encode_level(const FieldArgs &a, const LevelInfo &li, const float x01[3], float f[2]) {
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
    }
}

__device__ __forceinline__ int lane_level(int s, int q, int h) { return 8 * s + 4 * (q >> 1) + 2 * h + (q & 1); }

// --------------------------------------------------------- MLP forward
// MFMA A-operand (weight fragment) sources: LDS-staged fragments (whole or partial staging).
template <typename TM> struct LdsW {
    const TM *p;
    __device__ __forceinline__ typename FragT<TM>::T get(int id, int lane) const { return load_frag<TM>(p, id, lane); }
};
// LDS fragments read from one per-lane base address made opaque once per tile (fence() at the top of each
// tile of a loop), so every read is that base + a constant (the ds_read offset field): load_frag's per-read
// opaque index costs an s_mov and a v_lshl_add per read. The per-tile fence still keeps the reads inside the
// tile loop (hoisted, the fragments would take the registers). Fragment `id` sits at slot id - base.
template <typename TM> struct LdsWt {
    typedef __attribute__((address_space(3))) const char *LdsPtr;
    LdsPtr q;   // this lane's byte address of slot 0 minus base slots
    __device__ __forceinline__ LdsWt(const TM *p, int lane, int base = 0)
        : q((LdsPtr)(reinterpret_cast<const char *>(p) + ((int64_t)lane - (int64_t)base * 64) * 8 * (int64_t)sizeof(TM))) {}
    __device__ __forceinline__ void fence() { asm volatile("" : "+v"(q)); }
    __device__ __forceinline__ typename FragT<TM>::T get(int id, int) const {
        const LdsPtr a = q + id * 64 * 8 * (int)sizeof(TM);
        typename FragT<TM>::T f;
        if constexpr (sizeof(TM) == 2) {
            f = *reinterpret_cast<__attribute__((address_space(3))) const h8v *>(a);
        } else {
            typedef float f4e __attribute__((ext_vector_type(4)));
            typedef __attribute__((address_space(3))) const f4e *L4;
            const f4e x = *reinterpret_cast<L4>(a), y = *reinterpret_cast<L4>(a + 16);
            f.v[0] = x.x; f.v[1] = x.y; f.v[2] = x.z; f.v[3] = x.w; f.v[4] = y.x; f.v[5] = y.y; f.v[6] = y.z; f.v[7] = y.w;
        }
        return f;
    }
};

template <typename TM> struct Acts {
    typename FragT<TM>::T X[2], H1[2][2], Cin[2], H3[2][2], H4[2][2];
};

template <typename TM, typename W>
__device__ __forceinline__ void mlp_sdf_net(const W &wfr, const float *wb, Acts<TM> &A, int lane, float &sdf,
                                            f16v &l2) {
    const int h = lane >> 5;
    f16v acc[2];
    // L1: 32 -> 64, ReLU
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        acc_init_bias(acc[mt], wb + 0 * 64, mt, h);
#pragma unroll
        for (int s = 0; s < 2; ++s) mma(acc[mt], wfr.get(FR_L1 + mt * 2 + s, lane), A.X[s]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) acc_to_frag<TM>(acc[t], s, true, A.H1[t][s]);
    // L2: 64 -> 16 (sdf, geo[15])
    acc_init_bias(acc[0], wb + 1 * 64, 0, h);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) mma(acc[0], wfr.get(FR_L2 + 2 * t + s, lane), A.H1[t][s]);
    float sdf_v = acc[0][0];
    if constexpr (sizeof(TM) == 2) sdf_v = (float)(_Float16)sdf_v;   // fp16 Linear output under autocast
    sdf = __shfl(sdf_v, lane & 31, 64);                                 // row 0 lives in half 0
    l2 = acc[0];
}

// ReLU derivative of a 64-row activation as 32 bits (bit 16t + 8s + j)
template <typename TM>
__device__ __forceinline__ uint32_t relu_mask(const typename FragT<TM>::T (&H)[2][2]) {
    uint32_t m = 0;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if constexpr (sizeof(TM) == 2) {   // pair layout (pair_bits)
#pragma unroll
                for (int p = 0; p < 4; ++p) m |= pair_bits(h2v{H[t][s][2 * p], H[t][s][2 * p + 1]}, 8 * t + 4 * s + p);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) m |= (frag_get<TM>(H[t][s], j) > 0 ? 1u : 0u) << (16 * t + 8 * s + j);
            }
        }
    return m;
}

// Colour net on [geo, SH(view dir)] from the sigma net's L2 accumulator: fills A.Cin, A.H3, A.H4 and
// returns the 3 logits (all lanes, sample lane & 31) and, when `masks`, the ReLU masks of H3 / H4 to m3 / m4.
template <typename TM, typename W>
__device__ __forceinline__ void mlp_colour_net(const W &wfr, const float *wb, Acts<TM> &A, const f16v &l2,
                                               const typename FragT<TM>::T &shf, int lane, float logit[3], bool masks,
                                               uint32_t &m3, uint32_t &m4) {
    const int h = lane >> 5;
    f16v acc[2];
    // colour input: rows 0..15 = [sdf (zero weight), geo], rows 16..24 = SH (sh_frag)
    acc_to_frag<TM>(l2, 0, false, A.Cin[0]);
    A.Cin[1] = shf;
    // L3: 24 -> 64, ReLU
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        acc_init_bias(acc[mt], wb + 2 * 64, mt, h);
#pragma unroll
        for (int s = 0; s < 2; ++s) mma(acc[mt], wfr.get(FR_L3 + mt * 2 + s, lane), A.Cin[s]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) acc_to_frag<TM>(acc[t], s, true, A.H3[t][s]);
    if (masks) m3 = relu_mask<TM>(A.H3);
    // L4: 64 -> 64, ReLU
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        acc_init_bias(acc[mt], wb + 3 * 64, mt, h);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int s = 0; s < 2; ++s) mma(acc[mt], wfr.get(FR_L4 + mt * 4 + 2 * t + s, lane), A.H3[t][s]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) acc_to_frag<TM>(acc[t], s, true, A.H4[t][s]);
    if (masks) m4 = relu_mask<TM>(A.H4);
    // L5: 64 -> 3
    acc_init_bias(acc[0], wb + 4 * 64, 0, h);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) mma(acc[0], wfr.get(FR_L5 + 2 * t + s, lane), A.H4[t][s]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = acc[0][c];
        if constexpr (sizeof(TM) == 2) v = (float)(_Float16)v;
        logit[c] = __shfl(v, lane & 31, 64);
    }
}

// The colour net from a stored colour-net input fragment (k_encode SIG: the sigma net's L2 output
// rows 0..15 as fp16, exactly acc_to_frag(l2, 0) of mlp_colour_net)
template <typename TM, typename W>
__device__ __forceinline__ void mlp_colour_net_cin(const W &wfr, const float *wb, Acts<TM> &A,
                                                   const typename FragT<TM>::T &cin,
                                                   const typename FragT<TM>::T &shf, int lane, float logit[3]) {
    const int h = lane >> 5;
    f16v acc[2];
    A.Cin[0] = cin;
    A.Cin[1] = shf;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        acc_init_bias(acc[mt], wb + 2 * 64, mt, h);
#pragma unroll
        for (int s = 0; s < 2; ++s) mma(acc[mt], wfr.get(FR_L3 + mt * 2 + s, lane), A.Cin[s]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) acc_to_frag<TM>(acc[t], s, true, A.H3[t][s]);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        acc_init_bias(acc[mt], wb + 3 * 64, mt, h);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int s = 0; s < 2; ++s) mma(acc[mt], wfr.get(FR_L4 + mt * 4 + 2 * t + s, lane), A.H3[t][s]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) acc_to_frag<TM>(acc[t], s, true, A.H4[t][s]);
    acc_init_bias(acc[0], wb + 4 * 64, 0, h);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) mma(acc[0], wfr.get(FR_L5 + 2 * t + s, lane), A.H4[t][s]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = acc[0][c];
        if constexpr (sizeof(TM) == 2) v = (float)(_Float16)v;
        logit[c] = __shfl(v, lane & 31, 64);
    }
}

// ------------------------------------------------------ per-ray context
struct RayCtx {
    float dir[3], tgt[3], Rm[3][3], tv[3], vd[3];
    float depth, total;
    int frame, rtype;
    bool vdepth;
    const float *box;
    float ff[3];   // the frame's latent code (frame_features, n_ff <= 3 words; 0 past n_ff)
};
// Per-ray context record (k_ray_ctx, once per step): the fields of RayCtx in one 128-B row
// so the kernels' per-ray prologue is one batch of independent scalar loads instead of the
// dependent chain ray row -> frame -> pose row
constexpr int RCTX = 32;
__device__ __forceinline__ RayCtx build_ray(const FieldArgs &a, int r) {
    RayCtx c;
    const float *ray = a.rays + (size_t)r * 12;
#pragma unroll
    for (int i = 0; i < 3; ++i) { c.dir[i] = ray[i]; c.tgt[i] = ray[3 + i]; }
    c.depth = ray[6];
    c.frame = (int)ray[8];
    c.rtype = (int)ray[9];
    const float *T = a.tf + (size_t)c.frame * 16;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) c.Rm[i][j] = T[i * 4 + j];
        c.tv[i] = T[i * 4 + 3];
    }
    const float nrm = sqrtf((c.dir[0] * c.dir[0] + c.dir[1] * c.dir[1]) + c.dir[2] * c.dir[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) c.vd[i] = c.dir[i] / nrm;
    c.vdepth = (c.depth >= a.near_sc) && (c.depth <= a.far_sc);
    c.total = a.totals[r];
    c.box = a.intervals + (size_t)r * a.Kmax * 2;
#pragma unroll
    for (int i = 0; i < 3; ++i) c.ff[i] = i < a.n_ff ? a.ff[(size_t)c.frame * a.n_ff + i] : 0.f;
    return c;
}
// ray r's record (load_ray reads it back)
__device__ __forceinline__ void store_ray_ctx(float *rctx, int r, const RayCtx &c) {
    float4 *o = reinterpret_cast<float4 *>(rctx + (size_t)r * RCTX);
    o[0] = make_float4(c.dir[0], c.dir[1], c.dir[2], c.tgt[0]);
    o[1] = make_float4(c.tgt[1], c.tgt[2], c.Rm[0][0], c.Rm[0][1]);
    o[2] = make_float4(c.Rm[0][2], c.Rm[1][0], c.Rm[1][1], c.Rm[1][2]);
    o[3] = make_float4(c.Rm[2][0], c.Rm[2][1], c.Rm[2][2], c.tv[0]);
    o[4] = make_float4(c.tv[1], c.tv[2], c.vd[0], c.vd[1]);
    o[5] = make_float4(c.vd[2], c.depth, c.total, __int_as_float(c.frame));
    o[6] = make_float4(__int_as_float(c.rtype), c.ff[0], c.ff[1], c.ff[2]);
    o[7] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// every caller passes a wave-uniform ray: the record is read through the constant address
// space (scalar loads, the context stays in scalar registers)
// LATE: the record's address laundered by an empty asm, so a call inside a loop reloads the record
// (scalar-cache hits) instead of the compiler holding its fields in SGPRs across the loop
template <bool LATE = false>
__device__ __forceinline__ RayCtx load_ray(const FieldArgs &a, int r) {
    size_t addr = (size_t)(a.rctx + (size_t)r * RCTX);
    if (LATE) asm volatile("" : "+s"(addr));
    const ConstU32 q = (ConstU32)addr;
    auto f = [&](int i) { return __uint_as_float(q[i]); };
    RayCtx c;
#pragma unroll
    for (int i = 0; i < 3; ++i) { c.dir[i] = f(i); c.tgt[i] = f(3 + i); c.tv[i] = f(15 + i); c.vd[i] = f(18 + i); }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c.Rm[i][j] = f(6 + 3 * i + j);
    c.depth = f(21);
    c.total = f(22);
    c.frame = (int)q[23];
    c.rtype = (int)q[24];
#pragma unroll
    for (int i = 0; i < 3; ++i) c.ff[i] = f(25 + i);
    c.vdepth = (c.depth >= a.near_sc) && (c.depth <= a.far_sc);
    c.box = a.intervals + (size_t)r * a.Kmax * 2;
    return c;
}
// transform_pts (Utils.py:253-257) of p = dir * z; validity = inside [-1,1]^3 (run_network :1244)
__device__ __forceinline__ bool sample_point(const RayCtx &c, float z, float p[3], float x[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = c.dir[i] * z;
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = ((c.Rm[i][0] * p[0] + c.Rm[i][1] * p[1]) + c.Rm[i][2] * p[2]) + c.tv[i];
    return fabsf(x[0]) <= 1.f && fabsf(x[1]) <= 1.f && fabsf(x[2]) <= 1.f;
}

template <typename TM>
__device__ __forceinline__ void masked_frags(const f16v (&acc)[2], uint32_t m, typename FragT<TM>::T (&d)[2][2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if constexpr (sizeof(TM) == 2) {
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    frag_put2(d[t][s], p, pk_keep(pk_round(acc[t][8 * s + 2 * p], acc[t][8 * s + 2 * p + 1]), m,
                                                  8 * t + 4 * s + p));
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    frag_set<TM>(d[t][s], j, ((m >> (16 * t + 8 * s + j)) & 1u) ? acc[t][8 * s + j] : 0.f);
            }
        }
}

// G levels of one lane's sample encoded together: the base row and the 4 paired
// (x, x+1) loads of every level in the group are issued before any is consumed, then
// the trilinear sums run in encode_level's order (same results). Dense levels only
// take the paired loads; a hashed level falls back to encode_level.
// HALVES: the lane's level is lvs[k] of lane 0 in the wave's first half and that + 2 in the second
// (lane_level): the level record is then read by two wave-uniform (scalar) loads instead of a
// per-lane vector load ahead of the corner gathers
// LREC: the level records come from the wave's LDS table (level_table: per level {scale, res, off,
// hs} and {rs, rs^2, dense, 0}), one ds_read per record per lane — each lane half reads its own
// level's record (no per-half selects of scalar values, no dense test per lane, no SGPR pressure)
struct LevelRec { LevelInfo li; uint32_t rs, rs2, dense; };
__device__ __forceinline__ LevelRec level_rec(const uint4 *lvt, int lv) {
    const uint4 r0 = lvt[2 * lv], r1 = lvt[2 * lv + 1];
    return {{__uint_as_float(r0.x), r0.y, r0.z, r0.w}, r1.x, r1.y, r1.z};
}
// fill the wave's level table (lanes 0..15: one level each; levels past L read as hashed / not dense)
__device__ __forceinline__ void level_table(const FieldArgs &a, uint4 *lvt, int lane) {
    if (lane < 16) {
        LevelInfo li = {1.f, 0u, 0u, 0u};
        if (lane < (int)a.L) li = level_info(a, lane);
        const uint32_t rs = li.res + 1;
        const bool dn = lane < (int)a.L && level_dense(rs, li.hs);
        lvt[2 * lane] = make_uint4(__float_as_uint(li.scale), li.res, li.off, li.hs);
        lvt[2 * lane + 1] = make_uint4(rs, rs * rs, dn ? 1u : 0u, 0u);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}
template <typename TT, int G, bool HALVES = false, bool LREC = false>
__device__ __forceinline__ void encode_levels(const FieldArgs &a, const int (&lvs)[G], bool on, const float x01[3],
                                              float (&out)[G][2], const uint4 *lvt = nullptr) {
    const TT *tab = reinterpret_cast<const TT *>(a.table);
    float pos[G][3];
    uint32_t base[G], rs[G], rs2[G];
    bool dense[G];
    LevelInfo lis[G];
#pragma unroll
    for (int k = 0; k < G; ++k) {
        LevelInfo &li = lis[k];
        if constexpr (LREC) {
            const LevelRec rec = level_rec(lvt, lvs[k]);
            li = rec.li;
            rs[k] = rec.rs;
            rs2[k] = rec.rs2;
            dense[k] = on && rec.dense != 0u;
        } else {
            if constexpr (HALVES) {
                const int l0 = __builtin_amdgcn_readfirstlane(lvs[k]);
                const LevelInfo i0 = level_info_uniform(a, l0), i1 = level_info_uniform(a, l0 + 2);
                const bool hi = lvs[k] != l0;
                li = {hi ? i1.scale : i0.scale, hi ? i1.res : i0.res, hi ? i1.off : i0.off, hi ? i1.hs : i0.hs};
            } else {
                li = level_info(a, lvs[k]);
            }
            rs[k] = li.res + 1;
            rs2[k] = mul24(rs[k], rs[k]);
            dense[k] = on && lvs[k] < (int)a.L && level_dense_v(rs[k], li.hs);
        }
        uint32_t pg[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            // pos >= 0.5 for every in-box sample: truncation is the floor and v_fract_f32 the
            // exact pos - floor(pos) (off-box lanes' values are never used)
            pos[k][d] = __builtin_fmaf(x01[d], li.scale, 0.5f);
            pg[d] = (uint32_t)pos[k][d];
            pos[k][d] = __builtin_amdgcn_fractf(pos[k][d]);
        }
        base[k] = dense_base_v(li.off, pg, rs[k]);
    }
    typedef typename std::conditional<sizeof(TT) == 4, float4, uint2>::type Raw;
    Raw raw[G][4];
    const __amdgpu_buffer_rsrc_t trs = table_rsrc(a.table);
    if constexpr (sizeof(TT) == 2) {
        if (a.quads) {   // xy-quad mirror: the z and z+1 quads of the cell, two 16-B loads
            // unconditional, a lane whose level is not dense (or whose sample is off the box) reading quad 0:
            // its values are never used (the sums below skip it), and no zero-fill or exec mask per level
            const __amdgpu_buffer_rsrc_t qrs = table_rsrc(a.quads);
#pragma unroll
            for (int k = 0; k < G; ++k) {
                const uint32_t b0 = dense[k] ? base[k] : 0u, b1 = dense[k] ? base[k] + rs2[k] : 0u;
                const u4v q0 = __builtin_amdgcn_raw_buffer_load_b128(qrs, b0 * 16u, 0, 0);
                const u4v q1 = __builtin_amdgcn_raw_buffer_load_b128(qrs, b1 * 16u, 0, 0);
                raw[k][0] = make_uint2(q0.x, q0.y);
                raw[k][1] = make_uint2(q0.z, q0.w);
                raw[k][2] = make_uint2(q1.x, q1.y);
                raw[k][3] = make_uint2(q1.z, q1.w);
            }
            goto sums;
        }
    }
#pragma unroll
    for (int k = 0; k < G; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            raw[k][i] = Raw{};
            if (dense[k]) {
                const uint32_t row = base[k] + ((i & 1) ? rs[k] : 0u) + ((i & 2) ? rs2[k] : 0u);
                if constexpr (sizeof(TT) == 4) {
                    const TT *ptr = tab + (size_t)row * 2;
                    typedef float f4a __attribute__((ext_vector_type(4), aligned(8)));
                    const f4a v = *reinterpret_cast<const f4a *>(ptr);
                    raw[k][i] = make_float4(v.x, v.y, v.z, v.w);
                } else {
                    raw[k][i] = table_pair16(trs, row);
                }
            }
        }
sums:
#pragma unroll
    for (int k = 0; k < G; ++k) {
        out[k][0] = 0.f;
        out[k][1] = 0.f;
        if (!(on && lvs[k] < (int)a.L)) continue;
        if (!dense[k]) {
            encode_level<TT>(a, lis[k], x01, out[k]);
            continue;
        }
        if constexpr (sizeof(TT) == 2) {
            // fp16 corners: v_fma_mix_f32 takes each fp16 half straight from the loaded pair (the
            // exact f16 -> f32 widening inside the fma: the same result as convert + fma, without
            // the 16 conversions)
            float o0 = 0.f, o1 = 0.f;
#pragma unroll
            for (int idx = 0; idx < 8; ++idx) {
                float w = 1.f;
#pragma unroll
                for (int d = 0; d < 3; ++d) w *= ((idx >> d) & 1) ? pos[k][d] : 1 - pos[k][d];
                const uint32_t pr = (idx & 1) ? raw[k][idx >> 1].y : raw[k][idx >> 1].x;
                asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel_hi:[0,1,0]" : "+v"(o0) : "v"(w), "v"(pr));
                asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[0,1,0]" : "+v"(o1) : "v"(w), "v"(pr));
            }
            out[k][0] = o0;
            out[k][1] = o1;
        } else {
            float e[8][2];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                e[2 * i][0] = raw[k][i].x; e[2 * i][1] = raw[k][i].y;
                e[2 * i + 1][0] = raw[k][i].z; e[2 * i + 1][1] = raw[k][i].w;
            }
#pragma unroll
            for (int idx = 0; idx < 8; ++idx) {
                float w = 1.f;
#pragma unroll
                for (int d = 0; d < 3; ++d) w *= ((idx >> d) & 1) ? pos[k][d] : 1 - pos[k][d];
                out[k][0] = __builtin_fmaf(w, e[idx][0], out[k][0]);
                out[k][1] = __builtin_fmaf(w, e[idx][1], out[k][1]);
            }
        }
    }
}

// SH(view direction) rows 16..24 of the colour-net input as the second K-step
// B fragment (h0: SH0..3, SH8; h1: SH4..7) — one per ray.
// the view direction in the object frame (the SH input, run_network :1281)
__device__ __forceinline__ void view_dir(const RayCtx &c, float &x, float &y, float &z) {
    x = (c.Rm[0][0] * c.vd[0] + c.Rm[0][1] * c.vd[1]) + c.Rm[0][2] * c.vd[2];
    y = (c.Rm[1][0] * c.vd[0] + c.Rm[1][1] * c.vd[1]) + c.Rm[1][2] * c.vd[2];
    z = (c.Rm[2][0] * c.vd[0] + c.Rm[2][1] * c.vd[1]) + c.Rm[2][2] * c.vd[2];
}
__device__ __forceinline__ void sh_values(const RayCtx &c, float sh[9]) {
    float x, y, z;
    view_dir(c, x, y, z);
    const float xx = x * x, yy = y * y, zz = z * z;
    sh[0] = SH_C0; sh[1] = -SH_C1 * y; sh[2] = SH_C1 * z; sh[3] = -SH_C1 * x;
    sh[4] = SH_C2_0 * (x * y); sh[5] = SH_C2_1 * (y * z); sh[6] = SH_C2_2 * ((2.0f * zz - xx) - yy);
    sh[7] = SH_C2_3 * (x * z); sh[8] = SH_C2_4 * (xx - yy);
}
template <typename TM>
__device__ __forceinline__ typename FragT<TM>::T sh_frag(const RayCtx &c, int h, int n_ff = 0) {
    float sh[9];
    sh_values(c, sh);
    typename FragT<TM>::T f;
    frag_zero<TM>(f);
    if (h == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) frag_set<TM>(f, j, sh[j]);
        frag_set<TM>(f, 4, sh[8]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) frag_set<TM>(f, j, sh[4 + j]);
    }
    if (h == 0 && n_ff > 0) {   // frame features: Cin rows 25.. (from the ray's context record: scalar registers)
#pragma unroll
        for (int j = 0; j < 3; ++j) frag_set<TM>(f, 5 + j, c.ff[j]);
    }
    return f;
}

// ------------------------------------------------------------- staging
// Weight fragments FR0 .. FR0 + NFR - 1 ([64 lanes][8] TM each) and the bias image ([5][64] f32) at the start of
// a block's dynamic LDS, in that order; BIAS16 (the point query's colour pass under amp): a second bias image
// behind the first, rounded to fp16 as autocast rounds the bias. Kernel and launch share the layout:
// staged_bytes is the launch's LDS size (tail: bytes the kernel keeps behind the images), staged_bias the
// first bias image (the copy's s_b), NOF_STAGE_FRAGS the copy, without a barrier (each kernel places its
// own). A macro: inlined from a function the same loops changed the inference kernels' register counts.
constexpr int BIAS_WORDS = 5 * 64;
template <typename TM, int NFR>
__host__ __device__ constexpr size_t staged_bytes(bool bias16 = false, size_t tail = 0) {
    return (size_t)NFR * 64 * 8 * sizeof(TM) + (bias16 ? 2 : 1) * BIAS_WORDS * sizeof(float) + tail;
}
template <typename TM, int NFR>
__device__ __forceinline__ float *staged_bias(char *smem) {
    return reinterpret_cast<float *>(smem + NFR * 64 * 8 * sizeof(TM));
}
__device__ __forceinline__ float round_h(float v) { return (float)(_Float16)v; }
#define NOF_STAGE_FRAGS(TM, NFR, FR0, BIAS16, a, smem, s_b)                                                       \
    do {                                                                                                          \
        const uint4 *st_src = reinterpret_cast<const uint4 *>((a).frags) + (FR0) * 64 * 8 * (int)sizeof(TM) / 16; \
        uint4 *st_dst = reinterpret_cast<uint4 *>(smem);                                                          \
        for (int i = threadIdx.x; i < (NFR) * 64 * 8 * (int)sizeof(TM) / 16; i += blockDim.x) st_dst[i] = st_src[i]; \
        for (int i = threadIdx.x; i < BIAS_WORDS; i += blockDim.x) {                                              \
            (s_b)[i] = (a).bias[i];                                                                               \
            if constexpr (BIAS16) (s_b)[BIAS_WORDS + i] = round_h((a).bias[i]);                                   \
        }                                                                                                         \
    } while (0)

}  // namespace nof
