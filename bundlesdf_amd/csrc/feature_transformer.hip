// Feature transformer (include/nof.h group 12): the reference's LocalFeatureTransformer
// (BundleTrack/LoFTR/src/loftr/loftr_module/transformer.py with linear_attention.py's
// LinearAttention), the stage between a backbone and the matching head of group 11, as two fused
// kernels per layer application. The reference runs ~25 torch ops per application with [N,L,8,D]
// intermediates in memory; here a tile of 64 tokens goes through the whole layer on chip.
//
// Definition. One application x <- layer(x, source), x [L,C] and source [S,C] float32 in memory,
// H = 8 heads of D = C/8 channels, optional masks x_mask [L] and source_mask [S] (uint8, 0 = out):
//
//   Q = elu(x Wq^T) + 1         K = elu(source Wk^T) + 1        V = source Wv^T
//   Q *= x_mask                 K *= source_mask                V *= source_mask
//   KV_h = (1/S) sum_s K_h[s]^T V_h[s]  [D,D]       Ksum_h = sum_s K_h[s]  [D]
//   msg_h[l] = (Q_h[l] KV_h) * S / (Q_h[l] . Ksum_h + 1e-6)
//   m   = LayerNorm1(concat_h(msg) Wm^T)                   eps 1e-5, biased variance, affine
//   m   = LayerNorm2(relu([x | m] W1^T) W2^T)              W1 [2C,2C], W2 [C,2C], no biases
//   out = x + m
//
// S in the scaling is the full source length, not the number of unmasked rows. A stack applies its
// layers in order: "self" is a <- layer(a, a), b <- layer(b, b); "cross" is a <- layer(a, b), then
// b <- layer(b, a) with the a that has just been updated. The streams are updated in place.
//
// Numerics. Every product with a weight matrix, K^T V and Q KV is an MFMA (32x32x16) with fp16
// operands and float32 accumulation; elu, the masks, Z = Q . Ksum, the LayerNorm statistics (mean,
// then the mean of squared deviations, both summed in a fixed order), the affine terms and the
// residual add are float32. Values are rounded to fp16 exactly where they become an MFMA operand:
//   x and source (when a tile is staged), Q, K, V (after elu + 1 and the mask), KV (as the MEAN
//   over s, so it cannot overflow), msg (after the float32 factor S / (Z + 1e-6)), LayerNorm1's
//   output m, and the hidden layer relu([x | m] W1^T).
// Ksum is the float32 sum of the fp16-rounded K; Z is formed in float32 from the fp16-rounded Q and
// that Ksum, so a masked query (Q = 0) or a source with every row masked (Ksum = 0) gives Z = 0, the
// factor S / 1e-6 and a message of exactly 0: finite, as the reference in float64 (its fp16 path
// gives NaN there).
//
//  k_ft_kv     a block walks up to FT_KV_TILES tiles of 64 source rows: stages the tile as fp16,
//              projects K and V (tokens on the accumulator registers, channels on the lanes), writes
//              them transposed [channel][token] to LDS, and adds the tile's K^T V to accumulators
//              that live across the tiles: one 32x32 product per group of 32 channels (one head at
//              D = 32; two heads at D = 16, whose off-diagonal 16x16 blocks are dropped later). The
//              block's partial KV and Ksum go to the workspace.
//  k_ft_kvsum  sums the partials of a problem in block order, scales by 1/S, rounds to fp16 and writes
//              KV in the fragment order k_ft_layer's MFMA reads. No floating-point atomics: the same
//              bytes on every run, and a problem's result does not depend on the other problems.
//  k_ft_layer  a block owns 64 rows of x: Q projection, elu + 1, Z, Q KV, merge, LayerNorm1,
//              [x | m] W1^T, relu, W2^T, LayerNorm2, residual add. Channels on the accumulator
//              registers, tokens on the lanes, so a LayerNorm sum is a sum over a lane's registers plus
//              eight partials through LDS. Two LDS images of 64 rows x 2C fp16 hold [x | m] and
//              [Q | msg], later the hidden layer: 130 KB at C = 256. Global traffic is the x tile
//              (twice: staged, and again in float32 for the residual), the packed weights and the
//              output tile.
//
// Weights are packed on the host in the fragment order of mfma_tile.h, which also defines the lane /
// register layout of the tiles; the same fragment is the A operand in k_ft_layer and the B operand in
// k_ft_kv.
//
// Tails: a row past L or S is staged as zeros; its K and V are zeroed like a masked row's and its
// output is not written. There is no scalar path.
#include "mfma_tile.h"
#include "host_entry.h"

#pragma clang fp contract(off)

namespace nof {

constexpr int FT_ROWS = 64;                          // tokens of a tile
constexpr int FT_THREADS = 256;                      // four waves
constexpr int FT_KV_TILES = 4;                       // source tiles a k_ft_kv block sums in registers
constexpr int FT_KV_ROWS = FT_ROWS * FT_KV_TILES;
constexpr int FT_HEADS = 8;

struct FtSide {
    float *x;                  // [P,L,C] the stream that is updated
    const float *src;          // [P,S,C] its source
    const uint8_t *x_mask;     // [P,L] or null
    const uint8_t *src_mask;   // [P,S] or null
    int L, S;
};

struct FtArgs {
    FtSide side[2];            // problem q of a launch is pair q % P of side q / P
    int P;
    const h8v *wq, *wk, *wv, *wm, *w1, *w2;   // fragment order
    const float *ln;           // [4][C]: weight1, bias1, weight2, bias2
    float *part;               // [problems][max_blk][C 32 + C] partial KV and Ksum
    h8v *kv;                   // [problems][C/32][2][64] KV / S in fragment order
    float *ksum;               // [problems][C]
    int max_blk;
};

__device__ __forceinline__ float ft_elu1(float v) { return v > 0.f ? v + 1.0f : expf(v); }

template <int C>
__global__ void __launch_bounds__(FT_THREADS) k_ft_kv(const FtArgs a) {
    constexpr int NT = C / 128, KS = C / 16, XROW = 2 * C + ROW_PAD, TROW = 2 * FT_ROWS + ROW_PAD;
    __shared__ __attribute__((aligned(16))) unsigned char xs[FT_ROWS * XROW];
    __shared__ __attribute__((aligned(16))) unsigned char kt[C * TROW];
    __shared__ __attribute__((aligned(16))) unsigned char vt[C * TROW];
    __shared__ float keep[FT_ROWS];

    const int q = blockIdx.y, sd = q / a.P, p = q - sd * a.P;
    const FtSide &s = a.side[sd];
    const int S = s.S, row0 = blockIdx.x * FT_KV_ROWS;
    if (row0 >= S) return;
    const float *src = s.src + (size_t)p * S * C;
    const uint8_t *mask = s.src_mask ? s.src_mask + (size_t)p * S : nullptr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;

    f16v kv[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc_zero(kv[i]);
    float ksum = 0.f;                                // channel threadIdx.x (threads below C)

    for (int tile = 0; tile < FT_KV_TILES; ++tile) {
        const int t0 = row0 + tile * FT_ROWS;
        if (t0 >= S) break;
        __syncthreads();                             // the previous tile has been read
        stage_rows<C, FT_ROWS, FT_THREADS>(src, t0, S, xs, XROW);
        if (threadIdx.x < FT_ROWS) {
            const int t = t0 + threadIdx.x;
            keep[threadIdx.x] = (t < S && (mask == nullptr || mask[t] != 0)) ? 1.0f : 0.0f;
        }
        __syncthreads();

        f16v acc[NT][2];
        tile_gemm<NT, KS, true>(a.wk, NT * wave, xs, XROW, lane, acc);
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int chan = 32 * (NT * wave + i) + r, tok = 32 * t + acc_row(4 * g, h);
                    h4v o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (_Float16)(ft_elu1(acc[i][t][4 * g + e]) * keep[tok + e]);
                    *reinterpret_cast<h4v *>(kt + chan * TROW + tok * 2) = o;
                }
        tile_gemm<NT, KS, true>(a.wv, NT * wave, xs, XROW, lane, acc);
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int chan = 32 * (NT * wave + i) + r, tok = 32 * t + acc_row(4 * g, h);
                    h4v o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (_Float16)(acc[i][t][4 * g + e] * keep[tok + e]);
                    *reinterpret_cast<h4v *>(vt + chan * TROW + tok * 2) = o;
                }
        __syncthreads();

        // K^T V of the tile: rows d1 of K on the registers, columns d2 of V on the lanes, k = tokens
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int ks = 0; ks < FT_ROWS / 16; ++ks) {
                const int off = (32 * (NT * wave + i) + r) * TROW + ks * 32 + h * 16;   // as lds_operand
                mma(kv[i], *reinterpret_cast<const h8v *>(kt + off), *reinterpret_cast<const h8v *>(vt + off));
            }
        if (threadIdx.x < C) {
            const _Float16 *row = reinterpret_cast<const _Float16 *>(kt + threadIdx.x * TROW);
            float sum = 0.f;
            for (int t = 0; t < FT_ROWS; ++t) sum += (float)row[t];
            ksum += sum;
        }
    }

    float *part = a.part + ((size_t)q * a.max_blk + blockIdx.x) * (C * 32 + C);
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) part[(NT * wave + i) * 1024 + acc_row(e, h) * 32 + r] = kv[i][e];
    if (threadIdx.x < C) part[C * 32 + threadIdx.x] = ksum;
}

// one block per (group of 32 channels, problem): the partials in block order, 1/S, fp16, fragment order
template <int C>
__global__ void __launch_bounds__(FT_THREADS) k_ft_kvsum(const FtArgs a) {
    constexpr int D = C / FT_HEADS;
    const int g32 = blockIdx.x, q = blockIdx.y, sd = q / a.P;
    const int S = a.side[sd].S;
    const int nblk = (S + FT_KV_ROWS - 1) / FT_KV_ROWS;
    const float *part = a.part + (size_t)q * a.max_blk * (C * 32 + C);
    const float inv_s = 1.0f / (float)S;
    _Float16 *out = reinterpret_cast<_Float16 *>(a.kv + ((size_t)q * (C / 32) + g32) * 2 * 64);
    for (int idx = threadIdx.x; idx < 1024; idx += FT_THREADS) {
        const int d1 = idx >> 5, d2 = idx & 31;
        float sum = 0.f;
        for (int b = 0; b < nblk; ++b) sum += part[(size_t)b * (C * 32 + C) + g32 * 1024 + idx];
        if (d1 / D != d2 / D) sum = 0.f;             // D = 16: the product of two different heads
        const int ks = d1 >> 4, hh = (d1 >> 3) & 1, j = d1 & 7;
        out[((ks * 64) + hh * 32 + d2) * 8 + j] = (_Float16)(sum * inv_s);
    }
    if (threadIdx.x < 32) {
        const int chan = g32 * 32 + threadIdx.x;
        float sum = 0.f;
        for (int b = 0; b < nblk; ++b) sum += part[(size_t)b * (C * 32 + C) + C * 32 + chan];
        a.ksum[(size_t)q * C + chan] = sum;
    }
}

// LayerNorm over the channels of every token: acc[i][t] holds channels 32 (nt0 + i) + acc_row(e, h)
// (register e) of token 32 t + r. Partial sums of the eight (wave, half) pairs meet in red.
template <int NT, int C>
__device__ __forceinline__ void ft_layernorm(f16v (&acc)[NT][2], float (*red)[8][FT_ROWS], const float *gamma,
                                             const float *beta, int nt0, int wave, int lane) {
    const int r = lane & 31, h = lane >> 5;
    float mean[2], rstd[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) s += acc[i][t][e];
        red[0][wave * 2 + h][32 * t + r] = s;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += red[0][k][32 * t + r];
        mean[t] = s * (1.0f / C);
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float d = acc[i][t][e] - mean[t];
                v += d * d;
            }
        red[1][wave * 2 + h][32 * t + r] = v;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) v += red[1][k][32 * t + r];
        rstd[t] = 1.0f / sqrtf(v * (1.0f / C) + 1e-5f);
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int chan = 32 * (nt0 + i) + acc_row(e, h);
                acc[i][t][e] = (acc[i][t][e] - mean[t]) * rstd[t] * gamma[chan] + beta[chan];
            }
    }
}

template <int C>
__global__ void __launch_bounds__(FT_THREADS) k_ft_layer(const FtArgs a) {
    constexpr int NT = C / 128, KS = C / 16, D = C / FT_HEADS, AROW = 4 * C + ROW_PAD;
    __shared__ __attribute__((aligned(16))) unsigned char buf_a[FT_ROWS * AROW];   // [x | m]
    __shared__ __attribute__((aligned(16))) unsigned char buf_b[FT_ROWS * AROW];   // [Q | msg], then hidden
    __shared__ float red[2][8][FT_ROWS];
    __shared__ float zf[FT_ROWS][FT_HEADS];
    __shared__ float ksum[C];
    __shared__ float lnp[4 * C];
    __shared__ float keep[FT_ROWS];

    const int q = blockIdx.y, sd = q / a.P, p = q - sd * a.P;
    const FtSide &s = a.side[sd];
    const int L = s.L, row0 = blockIdx.x * FT_ROWS;
    if (row0 >= L) return;
    float *x = s.x + (size_t)p * L * C;
    const uint8_t *mask = s.x_mask ? s.x_mask + (size_t)p * L : nullptr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int nt0 = NT * wave;

    stage_rows<C, FT_ROWS, FT_THREADS>(x, row0, L, buf_a, AROW);
    for (int i = threadIdx.x; i < C; i += FT_THREADS) ksum[i] = a.ksum[(size_t)q * C + i];
    for (int i = threadIdx.x; i < 4 * C; i += FT_THREADS) lnp[i] = a.ln[i];
    if (threadIdx.x < FT_ROWS) {
        const int t = row0 + threadIdx.x;
        keep[threadIdx.x] = (t < L && (mask == nullptr || mask[t] != 0)) ? 1.0f : 0.0f;
    }
    __syncthreads();

    f16v acc[NT][2];
    // every epilogue: 4 consecutive channels of one token (registers 4 g .. 4 g + 3), 8 bytes into an LDS row
    auto chan_of = [&](int nt, int g) { return 32 * nt + acc_row(4 * g, h); };

    // Q = (elu(x Wq^T) + 1) x_mask -> buf_b[:, 0:C]
    tile_gemm<NT, KS, false>(a.wq, nt0, buf_a, AROW, lane, acc);
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int tok = 32 * t + r;
                *reinterpret_cast<h4v *>(buf_b + tok * AROW + chan_of(nt0 + i, g) * 2) =
                    acc_quad(acc[i][t], g, [&](float v, int) { return ft_elu1(v) * keep[tok]; });
            }
    __syncthreads();

    // the factor S / (Z + 1e-6) of every (token, head), Z in float32
    for (int idx = threadIdx.x; idx < FT_ROWS * FT_HEADS; idx += FT_THREADS) {
        const int tok = idx >> 3, hd = idx & 7;
        const _Float16 *qrow = reinterpret_cast<const _Float16 *>(buf_b + tok * AROW) + hd * D;
        float z = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) z += (float)qrow[d] * ksum[hd * D + d];
        zf[tok][hd] = (float)s.S / (z + 1e-6f);
    }
    __syncthreads();

    // msg = (Q KV / S) factor -> buf_b[:, C:2C]: tile nt of msg needs the 32 channels nt of Q only
    {
        const h8v *kv = a.kv + (size_t)q * (C / 32) * 2 * 64;
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                acc_zero(acc[i][t]);
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
                    mma(acc[i][t], packed_operand(kv, nt0 + i, 2, ks, lane),
                        lds_operand(buf_b + (nt0 + i) * 64, 32 * t + r, AROW, ks, h));
            }
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int tok = 32 * t + r, chan = chan_of(nt0 + i, g);
                    const float f = zf[tok][chan / D];           // 4 consecutive channels share a head
                    h4v o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (_Float16)(acc[i][t][4 * g + e] * f);
                    *reinterpret_cast<h4v *>(buf_b + tok * AROW + (C + chan) * 2) = o;
                }
    }
    __syncthreads();

    // m = LayerNorm1(msg Wm^T) -> buf_a[:, C:2C]
    tile_gemm<NT, KS, false>(a.wm, nt0, buf_b + 2 * C, AROW, lane, acc);
    ft_layernorm<NT, C>(acc, red, lnp, lnp + C, nt0, wave, lane);
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<h4v *>(buf_a + (32 * t + r) * AROW + (C + chan_of(nt0 + i, g)) * 2) =
                    acc_quad(acc[i][t], g, [](float v, int) { return v; });
    __syncthreads();

    // hidden = relu([x | m] W1^T) -> buf_b[:, 0:2C], two chunks of C channels
#pragma unroll 1
    for (int c = 0; c < 2; ++c) {
        const int n0 = (c * 4 + wave) * NT;
        tile_gemm<NT, 2 * KS, false>(a.w1, n0, buf_a, AROW, lane, acc);
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    *reinterpret_cast<h4v *>(buf_b + (32 * t + r) * AROW + chan_of(n0 + i, g) * 2) =
                        acc_quad(acc[i][t], g, [](float v, int) { return fmaxf(v, 0.f); });
    }
    __syncthreads();

    // out = x + LayerNorm2(hidden W2^T)
    tile_gemm<NT, 2 * KS, false>(a.w2, nt0, buf_b, AROW, lane, acc);
    ft_layernorm<NT, C>(acc, red, lnp + 2 * C, lnp + 3 * C, nt0, wave, lane);
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int tok = row0 + 32 * t + r;
            if (tok < L) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float4 *px = reinterpret_cast<float4 *>(x + (size_t)tok * C + chan_of(nt0 + i, g));
                    float4 v = *px;
                    v.x += acc[i][t][4 * g + 0];
                    v.y += acc[i][t][4 * g + 1];
                    v.z += acc[i][t][4 * g + 2];
                    v.w += acc[i][t][4 * g + 3];
                    *px = v;
                }
            }
        }
}

struct FtWs : Carver {
    float *part, *ksum;
    h8v *kv;
    int max_blk;
    FtWs(void *base, int32_t P, int32_t L, int32_t S, int32_t C) : Carver(base) {
        const size_t problems = 2 * (size_t)P;
        max_blk = (int)div_up((uint64_t)(L > S ? L : S), FT_KV_ROWS);
        part = take<float>(problems * max_blk * ((size_t)C * 32 + C));
        kv = take<h8v>(problems * (size_t)C * 32 / 8);
        ksum = take<float>(problems * (size_t)C);
    }
};

static size_t ft_layer_bytes(int32_t C) { return (size_t)20 * C * C + (size_t)16 * C; }

template <int C>
static void ft_apply(const FtArgs &a, int problems, int max_x, int max_src, hipStream_t s) {
    hipLaunchKernelGGL(k_ft_kv<C>, dim3(div_up(max_src, FT_KV_ROWS), (unsigned)problems), dim3(FT_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_ft_kvsum<C>, dim3(C / 32, (unsigned)problems), dim3(FT_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_ft_layer<C>, dim3(div_up(max_x, FT_ROWS), (unsigned)problems), dim3(FT_THREADS), 0, s, a);
}

}  // namespace nof

using namespace nof;

extern "C" {

size_t nof_feature_transformer_workspace_bytes(int32_t P, int32_t L, int32_t S, int32_t C) {
    if (P < 1 || 2 * (int64_t)P > 65535 || L < 1 || S < 1 || (C != 128 && C != 256)) return 0;
    return FtWs(nullptr, P, L, S, C).bytes;
}

int nof_feature_transformer(const nof_feature_transformer_desc *d, void *stream) {
    const char *fn = "feature_transformer";
    if (!d) return set_error(NOF_EINVAL, "%s: desc is NULL", fn);
    if (d->C != 128 && d->C != 256) return set_error(NOF_EINVAL, "%s: C=%d must be 128 or 256 (8 heads of 16 or 32)", fn, d->C);
    if (d->P < 1 || 2 * (int64_t)d->P > 65535) return set_error(NOF_EINVAL, "%s: P=%d must be in 1..32767", fn, d->P);
    if (d->L < 1) return set_error(NOF_EINVAL, "%s: L=%d must be at least 1", fn, d->L);
    if (d->S < 1) return set_error(NOF_EINVAL, "%s: S=%d must be at least 1", fn, d->S);
    if (d->n_layers < 1 || d->n_layers > NOF_FT_MAX_LAYERS)
        return set_error(NOF_EINVAL, "%s: n_layers=%d must be in 1..%d", fn, d->n_layers, NOF_FT_MAX_LAYERS);
    for (int l = 0; l < d->n_layers; ++l)
        if (d->layer_kind[l] != NOF_FT_SELF && d->layer_kind[l] != NOF_FT_CROSS)
            return set_error(NOF_EINVAL, "%s: layer_kind[%d]=%d must be NOF_FT_SELF or NOF_FT_CROSS", fn, l, d->layer_kind[l]);
    if (int rc = require_pointers(fn, {{d->feat_a, "feat_a"}, {d->feat_b, "feat_b"}, {d->weights, "weights"},
                                       {d->workspace, "workspace"}}))
        return rc;
    if (((uintptr_t)d->feat_a | (uintptr_t)d->feat_b | (uintptr_t)d->weights | (uintptr_t)d->workspace) & 15)
        return set_error(NOF_EINVAL, "%s: feat_a, feat_b, weights and workspace must be 16-byte aligned", fn);
    const size_t lb = ft_layer_bytes(d->C);
    if (d->weights_bytes < lb * d->n_layers)
        return set_error(NOF_EINVAL, "%s: weights_bytes=%zu is below the %zu bytes of %d layers", fn, d->weights_bytes,
                         lb * d->n_layers, d->n_layers);
    const FtWs ws(d->workspace, d->P, d->L, d->S, d->C);
    if (int rc = require_workspace(fn, d->workspace_bytes, ws.bytes)) return rc;

    hipStream_t s = (hipStream_t)stream;
    const int C = d->C;
    const FtSide aa{d->feat_a, d->feat_a, d->mask_a, d->mask_a, d->L, d->L};
    const FtSide bb{d->feat_b, d->feat_b, d->mask_b, d->mask_b, d->S, d->S};
    const FtSide ab{d->feat_a, d->feat_b, d->mask_a, d->mask_b, d->L, d->S};
    const FtSide ba{d->feat_b, d->feat_a, d->mask_b, d->mask_a, d->S, d->L};
    const int longest = d->L > d->S ? d->L : d->S;

    for (int l = 0; l < d->n_layers; ++l) {
        const char *w = static_cast<const char *>(d->weights) + lb * l;
        const size_t cc = (size_t)C * C * 2;
        FtArgs a{};
        a.P = d->P;
        a.wq = (const h8v *)w; a.wk = (const h8v *)(w + cc); a.wv = (const h8v *)(w + 2 * cc);
        a.wm = (const h8v *)(w + 3 * cc); a.w1 = (const h8v *)(w + 4 * cc); a.w2 = (const h8v *)(w + 8 * cc);
        a.ln = (const float *)(w + 10 * cc);
        a.part = ws.part; a.kv = ws.kv; a.ksum = ws.ksum; a.max_blk = ws.max_blk;
        auto apply = [&](int problems, int max_x, int max_src) {
            if (C == 128) ft_apply<128>(a, problems, max_x, max_src, s);
            else ft_apply<256>(a, problems, max_x, max_src, s);
        };
        if (d->layer_kind[l] == NOF_FT_SELF) {
            a.side[0] = aa; a.side[1] = bb;
            apply(2 * d->P, longest, longest);
        } else {
            a.side[0] = ab; a.side[1] = ab;
            apply(d->P, d->L, d->S);
            a.side[0] = ba; a.side[1] = ba;
            apply(d->P, d->S, d->L);
        }
    }
    return check_launch(fn);
}

}  // extern "C"
