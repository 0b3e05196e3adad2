// LoFTR backbone (include/nof.h group 14): the reference's ResNetFPN_8_2 (BundleTrack/LoFTR/src/loftr/
// backbone/resnet_fpn.py) in eval mode with initial_dim = 128 and block_dims = [128, 196, 256], from a grey
// image to the coarse tokens group 12 takes and the fine map group 13 takes. No other configuration.
//
// Definition.
//   x0 = relu(bn1(conv7x7 s2 p3 (1 -> 128)))                               1/2
//   layer1 = BasicBlock(128,128), BasicBlock(128,128)                      1/2   -> x1
//   layer2 = BasicBlock(128,196, s2), BasicBlock(196,196)                  1/4   -> x2
//   layer3 = BasicBlock(196,256, s2), BasicBlock(256,256)                  1/8   -> x3
//   BasicBlock: y = relu(bn1(conv3x3_s(x))); y = bn2(conv3x3(y)); out = relu(skip + y)
//               skip = x, or bn(conv1x1_s2(x)) when the stride is 2
//   x3_out = conv1x1(x3)                       256 -> 256                  coarse output
//   x2_out = conv3x3(lrelu(bn(conv3x3(conv1x1(x2) + up2(x3_out)))))  196->256, 256->256, 256->196
//   x1_out = conv3x3(lrelu(bn(conv3x3(conv1x1(x1) + up2(x2_out)))))  128->196, 196->196, 196->128   fine output
// No convolution has a bias; 3x3 convolutions pad 1; BatchNorm eps 1e-5; lrelu slope 0.01; up2 is the
// bilinear x2 upsample with align_corners=True.
//
// Layout. Activations are channels-last fp16 [N,h,w,C_p] in the caller's scratch buffer, C_p the channel
// count padded to a multiple of 32 (196 -> 224). Every pad channel holds exactly 0, in activations and in
// weights: a pad row of a matrix and its bias are 0, and relu, lrelu, up2 and the residual keep a 0.
//
// Weights (prepared on the host, bundlesdf_amd/backbone.py). BatchNorm is folded in float64: W' = W g /
// sqrt(var + eps) per output channel, rounded once to fp16; b' = beta - mean g / sqrt(var + eps) in float32
// (0 where no BatchNorm follows). A convolution is the matrix [Cout_p, K], K = taps Cin_p, k = (ky KW + kx)
// Cin_p + c, packed in mfma_tile.h's fragment order [Cout_p/32][K/16][64][8]. The stem has K = 49 padded
// with zeros to 64. conv2 of a down-sampling block carries its 1x1 stride-2 skip as Cin_p(block input)
// further columns after the 9 Cmid_p, and its b' is the sum of the two. The buffer holds the 20 layers of
// BB_LAYERS in order, each as its matrix followed by b' [Cout_p] f32, with no gaps; BbLayout states the
// offsets (every one a multiple of 128 bytes).
//
// Arithmetic. Every convolution is an implicit GEMM on v_mfma_f32_32x32x16_f16 with float32 accumulation:
// taps in (ky, kx) order, channels ascending within a tap, the fused skip after the last tap. The image is
// rounded to fp16 when the stem stages it. The epilogue is float32: + b', then the residual (fp16 read,
// added in f32), then the upsampled term, then relu or lrelu; the result is rounded once to fp16. No
// floating-point atomics and every sum runs in a fixed order: the same bytes on every run and for every
// split of the N images into calls.
//
// up2, from [h,w] to [2h,2w]: for output row y, sy = (float)(y (h - 1)) / (float)(2h - 1), y0 = floor(sy),
// y1 = min(y0 + 1, h - 1), fy = sy - y0, the same for x; the value is (1-fy)((1-fx) v00 + fx v01) +
// fy((1-fx) v10 + fx v11) in float32, in that order. At h = 1 every sy is 0.
//
// Outputs. coarse [N, hc wc, 256] float32 is x3_out before any rounding, plus pe [hc wc, 256] float32 in
// the same epilogue when pe != NULL: the token layout nof_feature_transformer takes. An fp16 copy of x3_out
// without pe feeds up2. fine [N, hf, wf, 128] fp16 channels-last is what nof_fine_windows reads.
//
//  k_stem   a block of four waves takes 8 x 8 outputs: stages the 21 x 21 image patch as fp16, every lane
//           gathers its pixel's 49 taps into four operands, wave n owns channels 32 n .. 32 n + 31.
//  k_conv<KH, STRIDE, EPILOGUE>  a block of four waves takes 8 x 8 outputs of one image and all output
//           channels: wave n owns the 32-channel tiles n and n + 4. Pixels lie on the lanes (pixel 32 t + r
//           of the tile, row-major, in accumulator t) and channels on the accumulator registers, so the
//           epilogue moves h4v quads into the channels-last output. The input patch with its halo is staged
//           in slices of 32 channels as fp16 rows of 2 * 32 + ROW_PAD = 80 bytes, out-of-image taps as zeros;
//           every tap reads its operand with lds_operand at a per-lane shifted row, weights come through
//           packed_operand (the largest matrix is 1.3 MB and stays in the L2). LDS, derived: the patch is
//           (7 STRIDE + KH)^2 rows, 17 x 17 x 80 = 23120 bytes at most (the stride-2 3x3; the whole 224
//           channels at once would take 134 KB of the CU's 160 KB), 8000 for a stride-1 3x3, 5120 for a
//           1x1, so LDS never bounds the blocks on a CU.
// 20 launches per call on the caller's stream; nothing is allocated or read back.
#include "mfma_tile.h"
#include "host_entry.h"

#pragma clang fp contract(off)

namespace nof {

constexpr int BB_THREADS = 256;                      // four waves
constexpr int BB_TILE = 8;                           // outputs a side of a block's tile
constexpr int BB_SLICE = 32;                         // channels staged at a time
constexpr int BB_ROW = 2 * BB_SLICE + ROW_PAD;       // bytes of a staged pixel
constexpr int BB_STEM_K = 64;                        // 49 taps padded
constexpr int BB_MAX_SIDE = 4096;
constexpr float BB_LRELU = 0.01f;

enum { EP_LINEAR = 0, EP_RELU = 1, EP_LRELU = 2, EP_UP = 3, EP_COARSE = 4 };

// cout, taps, cin, skip's cin (channels as the reference counts them)
struct BbLayer { int cout, taps, cin, skip; };
constexpr int BB_N_LAYERS = 20;
constexpr BbLayer BB_LAYERS[BB_N_LAYERS] = {
    {128, 49, 1, 0},                                                               // 0 conv1 + bn1
    {128, 9, 128, 0}, {128, 9, 128, 0}, {128, 9, 128, 0}, {128, 9, 128, 0},        // 1-4 layer1.{0,1}.{conv1,conv2}
    {196, 9, 128, 0}, {196, 9, 196, 128}, {196, 9, 196, 0}, {196, 9, 196, 0},      // 5-8 layer2 (6 with downsample)
    {256, 9, 196, 0}, {256, 9, 256, 196}, {256, 9, 256, 0}, {256, 9, 256, 0},      // 9-12 layer3 (10 with downsample)
    {256, 1, 256, 0},                                                              // 13 layer3_outconv
    {256, 1, 196, 0}, {256, 9, 256, 0}, {196, 9, 256, 0},                          // 14-16 layer2_outconv, _outconv2.{0,3}
    {196, 1, 128, 0}, {196, 9, 196, 0}, {128, 9, 196, 0},                          // 17-19 layer1_outconv, _outconv2.{0,3}
};
constexpr int bb_pad(int c) { return (c + 31) / 32 * 32; }
constexpr int bb_k(const BbLayer &l) { return l.taps == 49 ? BB_STEM_K : l.taps * bb_pad(l.cin) + bb_pad(l.skip); }

// byte offsets of every layer's matrix and bias in the weight buffer, and its size
struct BbLayout {
    size_t w[BB_N_LAYERS], b[BB_N_LAYERS], bytes;
    constexpr BbLayout() : w{}, b{}, bytes(0) {
        for (int i = 0; i < BB_N_LAYERS; ++i) {
            w[i] = bytes;
            bytes += (size_t)bb_pad(BB_LAYERS[i].cout) * bb_k(BB_LAYERS[i]) * 2;
            b[i] = bytes;
            bytes += (size_t)bb_pad(BB_LAYERS[i].cout) * 4;
        }
    }
};
constexpr BbLayout BB_LAYOUT{};

struct ConvArgs {
    const _Float16 *in;        // [N,Hi,Wi,Cin_p]
    const _Float16 *skip;      // [N,2 Ho,2 Wo,Cs_p] the block input of a fused 1x1 stride-2 skip, or null
    const h8v *w;              // [Cout_p, K] in fragment order
    const float *b;            // [Cout_p]
    _Float16 *out;             // [N,Ho,Wo,Cout_p]
    const _Float16 *res;       // EP_RELU: [N,Ho,Wo,Cout_p] or null
    const _Float16 *up;        // EP_UP: [N,Ho/2,Wo/2,Cout_p]
    float *coarse;             // EP_COARSE: [N,Ho Wo,Cout_p]
    const float *pe;           // EP_COARSE: [Ho Wo,Cout_p] or null
    int Hi, Wi, Cin_p, Cs_p;
    int Ho, Wo, Cout_p;
    int tiles_x, tiles_y;
};

// the block's tile: image n, first output (oy0, ox0)
__device__ __forceinline__ void bb_tile(int tiles_x, int tiles_y, int &n, int &oy0, int &ox0) {
    const int per = tiles_x * tiles_y;
    n = blockIdx.x / per;
    const int t = blockIdx.x - n * per;
    oy0 = (t / tiles_x) * BB_TILE;
    ox0 = (t % tiles_x) * BB_TILE;
}

// acc[i][t] += the KH x KH stride-S convolution of src [.,Hs,Ws,C_p] (image n) for the tile's pixels 32 t + r
// and the wave's output tiles nt[i], its k-steps starting at ks0 of the KS the matrix has. A 1x1 stages only
// the 64 pixels it reads. Ends with every wave past its last read of patch.
template <int KH, int S>
__device__ __forceinline__ void conv_accumulate(f16v (&acc)[2][2], const _Float16 *src, int n, int Hs, int Ws, int C_p,
                                                int oy0, int ox0, const h8v *__restrict__ w, int KS, int ks0, int nt0,
                                                int NT, unsigned char *patch) {
    constexpr int PS = KH == 1 ? 1 : S;              // patch pixels per output step
    constexpr int PW = 7 * PS + KH, PAD = KH / 2;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    int row0[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int p = 32 * t + r;
        row0[t] = (p >> 3) * PS * PW + (p & 7) * PS;
    }
    const int kpt = C_p / 16;                        // k-steps per tap
    for (int c0 = 0; c0 < C_p; c0 += BB_SLICE) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < PW * PW * 4; idx += BB_THREADS) {
            const int pix = idx >> 2, q = idx & 3;
            const int py = pix / PW, px = pix - py * PW;
            const int iy = KH == 1 ? (oy0 + py) * S : oy0 * S - PAD + py;
            const int ix = KH == 1 ? (ox0 + px) * S : ox0 * S - PAD + px;
            h8v v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (_Float16)0.f;
            if (iy >= 0 && iy < Hs && ix >= 0 && ix < Ws)
                v = *reinterpret_cast<const h8v *>(src + (((size_t)n * Hs + iy) * Ws + ix) * C_p + c0 + 8 * q);
            *reinterpret_cast<h8v *>(patch + pix * BB_ROW + 16 * q) = v;
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < KH * KH; ++tap) {
            const int shift = (tap / KH) * PW + tap % KH;
#pragma unroll
            for (int kk = 0; kk < BB_SLICE / 16; ++kk) {
                const int ks = ks0 + tap * kpt + c0 / 16 + kk;
                h8v x[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) x[t] = lds_operand(patch, row0[t] + shift, BB_ROW, kk, h);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if (nt0 + 4 * i < NT) {
                        const h8v wf = packed_operand(w, nt0 + 4 * i, KS, ks, lane);
#pragma unroll
                        for (int t = 0; t < 2; ++t) mma(acc[i][t], wf, x[t]);
                    }
                }
            }
        }
    }
}

// up2's two source rows (or columns) and weight of output index y from h sources
__device__ __forceinline__ void up2_coord(int y, int h, int &y0, int &y1, float &fy) {
    const float sy = (float)(y * (h - 1)) / (float)(2 * h - 1);
    y0 = (int)floorf(sy);
    y1 = y0 + 1 < h ? y0 + 1 : h - 1;
    fy = sy - (float)y0;
}

template <int KH, int STRIDE, int EPILOGUE>
__global__ void __launch_bounds__(BB_THREADS) k_conv(const ConvArgs a) {
    constexpr int PW = 7 * (KH == 1 ? 1 : STRIDE) + KH;
    __shared__ __attribute__((aligned(16))) unsigned char patch[PW * PW * BB_ROW];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    int n, oy0, ox0;
    bb_tile(a.tiles_x, a.tiles_y, n, oy0, ox0);
    const int NT = a.Cout_p / 32;
    const int KS = (KH * KH * a.Cin_p + (a.skip ? a.Cs_p : 0)) / 16;

    f16v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc_zero(acc[i][t]);
    conv_accumulate<KH, STRIDE>(acc, a.in, n, a.Hi, a.Wi, a.Cin_p, oy0, ox0, a.w, KS, 0, wave, NT, patch);
    if (EPILOGUE == EP_RELU && a.skip)
        conv_accumulate<1, 2>(acc, a.skip, n, 2 * a.Ho, 2 * a.Wo, a.Cs_p, oy0, ox0, a.w, KS, KH * KH * a.Cin_p / 16, wave, NT,
                              patch);

    // channels 32 nt + acc_row(., h) on the registers, the tile's pixel 32 t + r on the lanes
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int p = 32 * t + r, oy = oy0 + (p >> 3), ox = ox0 + (p & 7);
        if (oy >= a.Ho || ox >= a.Wo) continue;
        const size_t pix = ((size_t)n * a.Ho + oy) * a.Wo + ox;
        int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
        float fy = 0.f, fx = 0.f;
        const int hu = a.Ho / 2, wu = a.Wo / 2;
        if (EPILOGUE == EP_UP) {
            up2_coord(oy, hu, y0, y1, fy);
            up2_coord(ox, wu, x0, x1, fx);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int nt = wave + 4 * i;
            if (nt >= NT) continue;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int chan = 32 * nt + acc_row(4 * g, h);
                float v[4];
                if (EPILOGUE == EP_COARSE) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[i][t][4 * g + e];
                    float4 o = make_float4(v[0], v[1], v[2], v[3]);
                    if (a.pe) {
                        const float4 pe = *reinterpret_cast<const float4 *>(a.pe + ((size_t)oy * a.Wo + ox) * a.Cout_p + chan);
                        o = make_float4(v[0] + pe.x, v[1] + pe.y, v[2] + pe.z, v[3] + pe.w);
                    }
                    *reinterpret_cast<float4 *>(a.coarse + pix * a.Cout_p + chan) = o;
                } else {
                    const float4 b = *reinterpret_cast<const float4 *>(a.b + chan);
                    v[0] = acc[i][t][4 * g + 0] + b.x;
                    v[1] = acc[i][t][4 * g + 1] + b.y;
                    v[2] = acc[i][t][4 * g + 2] + b.z;
                    v[3] = acc[i][t][4 * g + 3] + b.w;
                }
                if (EPILOGUE == EP_RELU && a.res) {
                    const h4v rv = *reinterpret_cast<const h4v *>(a.res + pix * a.Cout_p + chan);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] + (float)rv[e];
                }
                if (EPILOGUE == EP_UP) {
                    const _Float16 *u = a.up + (size_t)n * hu * wu * a.Cout_p + chan;
                    const h4v v00 = *reinterpret_cast<const h4v *>(u + ((size_t)y0 * wu + x0) * a.Cout_p);
                    const h4v v01 = *reinterpret_cast<const h4v *>(u + ((size_t)y0 * wu + x1) * a.Cout_p);
                    const h4v v10 = *reinterpret_cast<const h4v *>(u + ((size_t)y1 * wu + x0) * a.Cout_p);
                    const h4v v11 = *reinterpret_cast<const h4v *>(u + ((size_t)y1 * wu + x1) * a.Cout_p);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float top = (1.f - fx) * (float)v00[e] + fx * (float)v01[e];
                        const float bot = (1.f - fx) * (float)v10[e] + fx * (float)v11[e];
                        v[e] = v[e] + ((1.f - fy) * top + fy * bot);
                    }
                }
                h4v o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float s = v[e];
                    if (EPILOGUE == EP_RELU) s = fmaxf(s, 0.f);
                    if (EPILOGUE == EP_LRELU) s = s > 0.f ? s : BB_LRELU * s;
                    o[e] = (_Float16)s;
                }
                *reinterpret_cast<h4v *>(a.out + pix * a.Cout_p + chan) = o;
            }
        }
    }
}

struct StemArgs {
    const float *images;       // [N,H,W]
    const h8v *w;              // [128,64] in fragment order
    const float *b;            // [128]
    _Float16 *out;             // [N,H/2,W/2,128]
    int H, W, Ho, Wo;
    int tiles_x, tiles_y;
};

__global__ void __launch_bounds__(BB_THREADS) k_stem(const StemArgs a) {
    constexpr int PW = 2 * 7 + 7, KS = BB_STEM_K / 16, C = 128;
    __shared__ _Float16 patch[PW * PW];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    int n, oy0, ox0;
    bb_tile(a.tiles_x, a.tiles_y, n, oy0, ox0);
    for (int idx = threadIdx.x; idx < PW * PW; idx += BB_THREADS) {
        const int py = idx / PW, px = idx - py * PW;
        const int iy = 2 * oy0 - 3 + py, ix = 2 * ox0 - 3 + px;
        float v = 0.f;
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = a.images[((size_t)n * a.H + iy) * a.W + ix];
        patch[idx] = (_Float16)v;
    }
    __syncthreads();

    f16v acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        acc_zero(acc[t]);
        const int p = 32 * t + r, base = 2 * (p >> 3) * PW + 2 * (p & 7);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            h8v x;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 16 * ks + 8 * h + j;               // tap ky 7 + kx; zeros past the 49
                x[j] = k < 49 ? patch[base + (k / 7) * PW + k % 7] : (_Float16)0.f;
            }
            mma(acc[t], packed_operand(a.w, wave, KS, ks, lane), x);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int p = 32 * t + r, oy = oy0 + (p >> 3), ox = ox0 + (p & 7);
        if (oy >= a.Ho || ox >= a.Wo) continue;
        _Float16 *out = a.out + (((size_t)n * a.Ho + oy) * a.Wo + ox) * C;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int chan = 32 * wave + acc_row(4 * g, h);
            const float4 b = *reinterpret_cast<const float4 *>(a.b + chan);
            const float bb[4] = {b.x, b.y, b.z, b.w};
            *reinterpret_cast<h4v *>(out + chan) = acc_quad(acc[t], g, [&](float v, int e) { return fmaxf(v + bb[e], 0.f); });
        }
    }
}

// The scratch buffer: three activations per level, reused as the comments say.
struct BbScratch : Carver {
    _Float16 *s0, *s1, *s2;    // 1/2: [128] x0, x1 | [224] conv1's outputs, layer1_outconv + up2 | [224] layer1.0's output, outconv2.0's
    _Float16 *m0, *m1, *m2;    // 1/4: [224] x2 | [256] conv1's outputs, layer2_outconv + up2, x2_out | [256] layer2.0's output, outconv2.0's
    _Float16 *c0, *c1, *c2;    // 1/8: [256] x3 | [256] conv1's outputs, x3_out | [256] layer3.0's output
    BbScratch(void *base, int64_t N, int64_t H, int64_t W) : Carver(base) {
        const size_t p2 = (size_t)(N * (H / 2) * (W / 2)), p4 = p2 / 4, p8 = p2 / 16;
        s0 = take<_Float16>(p2 * 128); s1 = take<_Float16>(p2 * 224); s2 = take<_Float16>(p2 * 224);
        m0 = take<_Float16>(p4 * 224); m1 = take<_Float16>(p4 * 256); m2 = take<_Float16>(p4 * 256);
        c0 = take<_Float16>(p8 * 256); c1 = take<_Float16>(p8 * 256); c2 = take<_Float16>(p8 * 256);
    }
};

// NOF_OK, or the refusal of a shape; the stem's grid is the largest of the call
static int bb_shape(const char *fn, int64_t N, int64_t H, int64_t W) {
    if (N < 1) return set_error(NOF_EINVAL, "%s: N=%lld must be at least 1", fn, (long long)N);
    if (H < 8 || H % 8 || H > BB_MAX_SIDE)
        return set_error(NOF_EINVAL, "%s: H=%lld must be a multiple of 8 in 8..%d", fn, (long long)H, BB_MAX_SIDE);
    if (W < 8 || W % 8 || W > BB_MAX_SIDE)
        return set_error(NOF_EINVAL, "%s: W=%lld must be a multiple of 8 in 8..%d", fn, (long long)W, BB_MAX_SIDE);
    if (N * div_up(H / 2, BB_TILE) * div_up(W / 2, BB_TILE) > 0x7fffffffLL)
        return set_error(NOF_EINVAL, "%s: N=%lld images of %lldx%lld are more than 2^31 - 1 tiles", fn, (long long)N,
                         (long long)H, (long long)W);
    return NOF_OK;
}

// one convolution layer li from `in` [N,Hi,Wi,.] to `out` [N,Ho,Wo,.]
template <int KH, int STRIDE, int EPILOGUE>
static void bb_conv(hipStream_t s, const char *weights, int li, int N, const _Float16 *in, int Hi, int Wi, _Float16 *out,
                    const _Float16 *skip = nullptr, const _Float16 *res = nullptr, const _Float16 *up = nullptr,
                    float *coarse = nullptr, const float *pe = nullptr) {
    const BbLayer &l = BB_LAYERS[li];
    ConvArgs a{};
    a.in = in; a.skip = skip; a.out = out; a.res = res; a.up = up; a.coarse = coarse; a.pe = pe;
    a.w = (const h8v *)(weights + BB_LAYOUT.w[li]);
    a.b = (const float *)(weights + BB_LAYOUT.b[li]);
    a.Hi = Hi; a.Wi = Wi; a.Cin_p = bb_pad(l.cin); a.Cs_p = bb_pad(l.skip);
    a.Ho = Hi / STRIDE; a.Wo = Wi / STRIDE; a.Cout_p = bb_pad(l.cout);
    a.tiles_x = div_up(a.Wo, BB_TILE); a.tiles_y = div_up(a.Ho, BB_TILE);
    hipLaunchKernelGGL((k_conv<KH, STRIDE, EPILOGUE>), dim3((uint32_t)N * a.tiles_x * a.tiles_y), dim3(BB_THREADS), 0, s, a);
}

}  // namespace nof

using namespace nof;

extern "C" {

size_t nof_backbone_weights_bytes(void) { return BB_LAYOUT.bytes; }

size_t nof_backbone_scratch_bytes(int32_t N, int32_t H, int32_t W) {
    if (bb_shape("backbone_scratch_bytes", N, H, W)) return 0;
    return BbScratch(nullptr, N, H, W).bytes;
}

int nof_backbone(const nof_backbone_desc *d, void *stream) {
    const char *fn = "backbone";
    if (!d) return set_error(NOF_EINVAL, "%s: desc is NULL", fn);
    if (int rc = bb_shape(fn, d->N, d->H, d->W)) return rc;
    const NamedPointer ptrs[] = {{d->images, "images"}, {d->weights, "weights"}, {d->pe, "pe", false}, {d->coarse, "coarse"},
                                 {d->fine, "fine"}, {d->scratch, "scratch"}};
    for (const NamedPointer &p : ptrs) {
        if (int rc = require_pointers(fn, {p})) return rc;
        if ((uintptr_t)p.p & 15) return set_error(NOF_EINVAL, "%s: %s must be 16-byte aligned", fn, p.name);
    }
    if (int rc = require_workspace(fn, d->weights_bytes, BB_LAYOUT.bytes, "weights_bytes")) return rc;
    if (int rc = require_workspace(fn, d->scratch_bytes, BbScratch(nullptr, d->N, d->H, d->W).bytes, "scratch_bytes")) return rc;

    const BbScratch ws(d->scratch, d->N, d->H, d->W);
    const char *w = static_cast<const char *>(d->weights);
    hipStream_t s = (hipStream_t)stream;
    const int N = d->N, h2 = d->H / 2, w2 = d->W / 2, h4 = h2 / 2, w4 = w2 / 2, h8 = h4 / 2, w8 = w4 / 2;
    _Float16 *fine = static_cast<_Float16 *>(d->fine);

    StemArgs st{d->images, (const h8v *)(w + BB_LAYOUT.w[0]), (const float *)(w + BB_LAYOUT.b[0]), ws.s0, d->H, d->W, h2, w2,
                (int)div_up(w2, BB_TILE), (int)div_up(h2, BB_TILE)};
    hipLaunchKernelGGL(k_stem, dim3((uint32_t)N * st.tiles_x * st.tiles_y), dim3(BB_THREADS), 0, s, st);
    // layer1: x0 = s0 -> s2 (block 0) -> x1 = s0
    bb_conv<3, 1, EP_RELU>(s, w, 1, N, ws.s0, h2, w2, ws.s1);
    bb_conv<3, 1, EP_RELU>(s, w, 2, N, ws.s1, h2, w2, ws.s2, nullptr, ws.s0);
    bb_conv<3, 1, EP_RELU>(s, w, 3, N, ws.s2, h2, w2, ws.s1);
    bb_conv<3, 1, EP_RELU>(s, w, 4, N, ws.s1, h2, w2, ws.s0, nullptr, ws.s2);
    // layer2: x1 = s0 -> m2 (block 0, the skip from x1) -> x2 = m0
    bb_conv<3, 2, EP_RELU>(s, w, 5, N, ws.s0, h2, w2, ws.m1);
    bb_conv<3, 1, EP_RELU>(s, w, 6, N, ws.m1, h4, w4, ws.m2, ws.s0);
    bb_conv<3, 1, EP_RELU>(s, w, 7, N, ws.m2, h4, w4, ws.m1);
    bb_conv<3, 1, EP_RELU>(s, w, 8, N, ws.m1, h4, w4, ws.m0, nullptr, ws.m2);
    // layer3: x2 = m0 -> c2 (block 0, the skip from x2) -> x3 = c0
    bb_conv<3, 2, EP_RELU>(s, w, 9, N, ws.m0, h4, w4, ws.c1);
    bb_conv<3, 1, EP_RELU>(s, w, 10, N, ws.c1, h8, w8, ws.c2, ws.m0);
    bb_conv<3, 1, EP_RELU>(s, w, 11, N, ws.c2, h8, w8, ws.c1);
    bb_conv<3, 1, EP_RELU>(s, w, 12, N, ws.c1, h8, w8, ws.c0, nullptr, ws.c2);
    // x3_out = c1 (fp16) and coarse; x2_out = m1; fine
    bb_conv<1, 1, EP_COARSE>(s, w, 13, N, ws.c0, h8, w8, ws.c1, nullptr, nullptr, nullptr, d->coarse, d->pe);
    bb_conv<1, 1, EP_UP>(s, w, 14, N, ws.m0, h4, w4, ws.m1, nullptr, nullptr, ws.c1);
    bb_conv<3, 1, EP_LRELU>(s, w, 15, N, ws.m1, h4, w4, ws.m2);
    bb_conv<3, 1, EP_LINEAR>(s, w, 16, N, ws.m2, h4, w4, ws.m1);
    bb_conv<1, 1, EP_UP>(s, w, 17, N, ws.s0, h2, w2, ws.s1, nullptr, nullptr, ws.m1);
    bb_conv<3, 1, EP_LRELU>(s, w, 18, N, ws.s1, h2, w2, ws.s2);
    bb_conv<3, 1, EP_LINEAR>(s, w, 19, N, ws.s2, h2, w2, fine);
    return check_launch(fn);
}

}  // extern "C"
