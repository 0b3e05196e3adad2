// Fine-level match refinement (include/nof.h group 13): the reference's FinePreprocess
// (BundleTrack/LoFTR/src/loftr/loftr_module/fine_preprocess.py) and FineMatching
// (BundleTrack/LoFTR/src/loftr/utils/fine_matching.py), the two stages around its fine transformer
// (loftr_fine, which is group 12's nof_feature_transformer at C = 128 called on the windows in place).
// The reference unfolds a 5x5 window around EVERY coarse cell of both maps ([N, L, 25, 128] each) and
// then indexes the matches; here only the windows of the matches are ever formed.
//
// Definition (W = 5, WW = 25, C = 128 fine channels, 256 coarse channels). For match m with pair p =
// pair[m], cell i = i[m] of A's coarse grid (h0, w0) and cell j = j[m] of B's (h1, w1); side A reads the
// fine map frames_a[p] (p itself without frames_a), a channels-last fp16 [stride h0, stride w0, 128]:
//
//   fine_window[r]  = the fine feature at (stride (i / w0) + ky - 2, stride (i % w0) + kx - 2),
//                     r = 5 ky + kx, zeros outside the map                                  [25,128]
//   ctx             = Wd coarse[p, i] + b_down                                              [128]
//   win[r]          = Wm[:, :128] fine_window[r] + (Wm[:, 128:] ctx + b_merge)              [25,128]
// and side B the same around j. After the transformer has turned (win_A, win_B) into (f0, f1):
//   sim[r]  = f0[12] . f1[r] / sqrt(128),  heat = softmax_r(sim)
//   x = sum_r heat[r] gx[r],  y = sum_r heat[r] gy[r],   gx = -1 + kx / 2, gy = -1 + ky / 2
//   std = sqrt(max(sum heat gx^2 - x^2, 1e-10)) + sqrt(max(sum heat gy^2 - y^2, 1e-10))
//   expec[m] = (x, y, std)
//
// Numerics. The three matrix products (Wd, Wm[:, 128:], Wm[:, :128]) are MFMAs (32x32x16) with fp16
// operands and float32 accumulation. Values are rounded to fp16 exactly where they become an MFMA
// operand:
//   the coarse row (float32 in memory, when a tile is staged) and Wd coarse + b_down (after the bias
//   has been added in float32). The fine map is fp16 in memory and is not rounded again; the weights
//   were rounded once on the host.
// b_down, b_merge and the context vector are added in float32 and win is written as float32. The
// correlation is a float32 dot product of the float32 rows the transformer left in memory (nothing is
// rounded to fp16 after the transformer), each lane two channels, summed over the wave by a butterfly
// whose order is fixed; the scale 1/sqrt(128), exp, the division by the sum and the moments (each a sum
// over r = 0..24 in order) are float32. No floating-point atomics: the same bytes on every run, and a
// match's result does not depend on the other matches of the call.
//
//  k_fine_context  a block takes 32 rows of the [2M] list (side A's M matches, then side B's): gathers
//                  their coarse rows by (pair, cell), stages them as fp16, and chains the two products,
//                  256 -> 128 and 128 -> 128, through LDS; wave n owns output channels 32 n .. 32 n + 31,
//                  channels on the accumulator registers and rows on the lanes. Writes ctx [2M,128] f32.
//  k_fine_windows  a wave takes one window as a 32-row tile with 25 live rows: lane (r, half) reads row
//                  r's 8 fp16 of every k-step straight from the fine map as the MFMA's B operand, so
//                  nothing goes through LDS. Wm[:, :128] stays in registers (32 fragments per lane, in
//                  the fragment order of mfma_tile.h) while the block loops over windows. Adds ctx and
//                  writes float32 [M,25,128] per side: what nof_feature_transformer updates in place.
//  k_fine_expect   a wave per match: 25 dot products, the softmax and the moments.
//
// Indices come from device memory: every kernel checks pair against P and the cells against their grids
// (k_fine_windows also the frame against N) before it forms an address. A row that fails is written as
// zeros (context, window and expec alike) and nothing is read for it.
#include "mfma_tile.h"
#include "host_entry.h"

#pragma clang fp contract(off)

namespace nof {

constexpr int FM_C = 128;                            // fine channels
constexpr int FM_CC = 256;                           // coarse channels
constexpr int FM_WW = 25;                            // rows of a window
constexpr int FM_THREADS = 256;                      // four waves
constexpr int FM_CTX_ROWS = 32;                      // rows of a k_fine_context tile
constexpr int FM_MAX_BLOCKS = 2048;                  // k_fine_windows: blocks that loop over the windows

struct FmArgs {
    const _Float16 *fine[2];   // [N,stride h,stride w,128]
    const float *coarse[2];    // [P,h w,256]
    const int32_t *frames[2];  // [P] or null
    const int32_t *pair;       // [M]
    const int32_t *cell[2];    // i, j [M]
    int M, P;
    int N[2], h[2], w[2];
    int stride;
    const h8v *w_down, *w_fine, *w_ctx;    // fragment order (mfma_tile.h)
    const float *b_down, *b_merge;
    float *ctx;                // [2M,128]
    float *win[2];             // [M,25,128]
};

// pair and cell of match m on side sd; false if either is out of range
__device__ __forceinline__ bool fm_row(const int32_t *pair, const int32_t *cell, int m, int P, int cells, int &p, int &c) {
    p = pair[m];
    c = cell[m];
    return p >= 0 && p < P && c >= 0 && c < cells;
}

__global__ void __launch_bounds__(FM_THREADS) k_fine_context(const FmArgs a) {
    constexpr int XROW = 2 * FM_CC + ROW_PAD, YROW = 2 * FM_C + ROW_PAD;
    __shared__ __attribute__((aligned(16))) unsigned char xs[FM_CTX_ROWS * XROW];   // coarse rows, fp16
    __shared__ __attribute__((aligned(16))) unsigned char ys[FM_CTX_ROWS * YROW];   // Wd coarse + b_down, fp16
    __shared__ int ok[FM_CTX_ROWS];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * FM_CTX_ROWS, rows = 2 * a.M;

    {   // eight threads stage one row: 32 channels each
        const int row = threadIdx.x >> 3, part = threadIdx.x & 7, q = q0 + row;
        const float *src = nullptr;
        if (q < rows) {
            const int sd = q >= a.M ? 1 : 0, m = q - sd * a.M, cells = a.h[sd] * a.w[sd];
            int p, c;
            if (fm_row(a.pair, a.cell[sd], m, a.P, cells, p, c)) src = a.coarse[sd] + ((size_t)p * cells + c) * FM_CC;
        }
        if (part == 0) ok[row] = src != nullptr;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c4 = part * 8 + k;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (src) v = *reinterpret_cast<const float4 *>(src + c4 * 4);
            const h4v o = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
            *reinterpret_cast<h4v *>(xs + row * XROW + c4 * 8) = o;
        }
    }
    __syncthreads();

    // channels 32 wave + acc_row(., h) on the registers (8 g + 4 h = acc_row(4 g, h)), the tile's rows on the lanes
    f16v acc;
    acc_zero(acc);
#pragma unroll
    for (int ks = 0; ks < FM_CC / 16; ++ks)
        mma(acc, packed_operand(a.w_down, wave, FM_CC / 16, ks, lane), lds_operand(xs, r, XROW, ks, h));
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int chan = 32 * wave + 8 * g + 4 * h;
        const float4 b = *reinterpret_cast<const float4 *>(a.b_down + chan);
        const h4v o = {(_Float16)(acc[4 * g + 0] + b.x), (_Float16)(acc[4 * g + 1] + b.y),
                       (_Float16)(acc[4 * g + 2] + b.z), (_Float16)(acc[4 * g + 3] + b.w)};
        *reinterpret_cast<h4v *>(ys + r * YROW + chan * 2) = o;
    }
    __syncthreads();

    acc_zero(acc);
#pragma unroll
    for (int ks = 0; ks < FM_C / 16; ++ks)
        mma(acc, packed_operand(a.w_ctx, wave, FM_C / 16, ks, lane), lds_operand(ys, r, YROW, ks, h));
    const int q = q0 + r;
    if (q < rows) {
        const bool live = ok[r] != 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int chan = 32 * wave + 8 * g + 4 * h;
            const float4 b = *reinterpret_cast<const float4 *>(a.b_merge + chan);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) v = make_float4(acc[4 * g + 0] + b.x, acc[4 * g + 1] + b.y, acc[4 * g + 2] + b.z, acc[4 * g + 3] + b.w);
            *reinterpret_cast<float4 *>(a.ctx + (size_t)q * FM_C + chan) = v;
        }
    }
}

__global__ void __launch_bounds__(FM_THREADS, 2) k_fine_windows(const FmArgs a) {
    constexpr int NT = FM_C / 32, KS = FM_C / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int ky = r / 5, kx = r - 5 * ky;           // rows 25 .. 31 of the tile are not live

    h8v wm[NT][KS];                                  // Wm[:, :128], once per block
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) wm[nt][ks] = packed_operand(a.w_fine, nt, KS, ks, lane);

    const int rows = 2 * a.M;
    for (int q = blockIdx.x * 4 + wave; q < rows; q += gridDim.x * 4) {
        const int sd = q >= a.M ? 1 : 0, m = q - sd * a.M;
        const int hc = a.h[sd], wc = a.w[sd];
        float *out = a.win[sd] + (size_t)m * (FM_WW * FM_C);
        int p, c, f = 0;
        bool good = fm_row(a.pair, a.cell[sd], m, a.P, hc * wc, p, c);
        if (good) {
            f = a.frames[sd] ? a.frames[sd][p] : p;
            good = f >= 0 && f < a.N[sd];
        }
        if (!good) {
            for (int idx = lane; idx < FM_WW * FM_C / 4; idx += 64)
                reinterpret_cast<float4 *>(out)[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const int hf = a.stride * hc, wf = a.stride * wc;
        const int cy = c / wc, cx = c - cy * wc;
        const int y = a.stride * cy + ky - 2, x = a.stride * cx + kx - 2;
        const bool live = r < FM_WW && y >= 0 && y < hf && x >= 0 && x < wf;

        h8v xf[KS];
        if (live) {
            const _Float16 *px = a.fine[sd] + (((size_t)f * hf + y) * wf + x) * FM_C + 8 * h;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) xf[ks] = *reinterpret_cast<const h8v *>(px + 16 * ks);
        } else {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int e = 0; e < 8; ++e) xf[ks][e] = (_Float16)0.f;
        }
        f16v acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc_zero(acc[nt]);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) mma(acc[nt], wm[nt][ks], xf[ks]);

        // channels 32 nt + acc_row(., h) on the registers, window row r on the lanes
        if (r < FM_WW) {
            const float *ctx = a.ctx + (size_t)q * FM_C;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int chan = 32 * nt + acc_row(4 * g, h);
                    const float4 cv = *reinterpret_cast<const float4 *>(ctx + chan);
                    const float4 v = make_float4(acc[nt][4 * g + 0] + cv.x, acc[nt][4 * g + 1] + cv.y,
                                                 acc[nt][4 * g + 2] + cv.z, acc[nt][4 * g + 3] + cv.w);
                    *reinterpret_cast<float4 *>(out + r * FM_C + chan) = v;
                }
        }
    }
}

struct FeArgs {
    const float *win_a, *win_b;   // [M,25,128]
    const int32_t *pair, *i, *j;  // [M]
    int M, P, L, S;
    float *expec;                 // [M,3]
};

__global__ void __launch_bounds__(FM_THREADS) k_fine_expect(const FeArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = blockIdx.x * 4 + wave;
    if (m >= a.M) return;
    int p, ci, cj;
    const bool good = fm_row(a.pair, a.i, m, a.P, a.L, p, ci) && fm_row(a.pair, a.j, m, a.P, a.S, p, cj);
    if (!good) {
        if (lane < 3) a.expec[(size_t)m * 3 + lane] = 0.f;
        return;
    }
    // lane l holds channels 2 l, 2 l + 1; the butterfly leaves the same sum on every lane
    const float2 c0 = reinterpret_cast<const float2 *>(a.win_a + ((size_t)m * FM_WW + FM_WW / 2) * FM_C)[lane];
    const float2 *rows = reinterpret_cast<const float2 *>(a.win_b + (size_t)m * FM_WW * FM_C);
    float sim[FM_WW];
#pragma unroll
    for (int r = 0; r < FM_WW; ++r) {
        const float2 v = rows[r * (FM_C / 2) + lane];
        float s = c0.x * v.x + c0.y * v.y;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        sim[r] = s * 0.08838834764831845f;           // 1 / sqrt(128)
    }
    float mx = sim[0];
#pragma unroll
    for (int r = 1; r < FM_WW; ++r) mx = fmaxf(mx, sim[r]);
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < FM_WW; ++r) {
        sim[r] = expf(sim[r] - mx);
        sum += sim[r];
    }
    float ex = 0.f, ey = 0.f, exx = 0.f, eyy = 0.f;
#pragma unroll
    for (int r = 0; r < FM_WW; ++r) {
        const float heat = sim[r] / sum;
        const float gx = -1.0f + 0.5f * (float)(r % 5), gy = -1.0f + 0.5f * (float)(r / 5);
        ex += heat * gx;
        ey += heat * gy;
        exx += heat * (gx * gx);
        eyy += heat * (gy * gy);
    }
    const float sd = sqrtf(fmaxf(exx - ex * ex, 1e-10f)) + sqrtf(fmaxf(eyy - ey * ey, 1e-10f));
    if (lane == 0) {
        a.expec[(size_t)m * 3 + 0] = ex;
        a.expec[(size_t)m * 3 + 1] = ey;
        a.expec[(size_t)m * 3 + 2] = sd;
    }
}

constexpr int FM_MAX_M = 1 << 24;
constexpr int FM_MAX_SIDE = 32768;                   // stride h, stride w
static size_t fm_weight_bytes() { return (size_t)2 * FM_C * FM_CC * 2 + (size_t)2 * FM_C * 4; }

static int fm_indices(const char *fn, int32_t M, int32_t P, const void *pair, const void *i, const void *j) {
    if (M < 0 || M > FM_MAX_M) return set_error(NOF_EINVAL, "%s: M=%d must be in 0..%d", fn, M, FM_MAX_M);
    if (P < 1) return set_error(NOF_EINVAL, "%s: P=%d must be at least 1", fn, P);
    if (M > 0) {
        if (!pair) return set_error(NOF_EINVAL, "%s: pair is NULL", fn);
        if (!i) return set_error(NOF_EINVAL, "%s: i is NULL", fn);
        if (!j) return set_error(NOF_EINVAL, "%s: j is NULL", fn);
    }
    return NOF_OK;
}

}  // namespace nof

using namespace nof;

extern "C" {

int nof_fine_windows(const nof_fine_windows_desc *d, void *stream) {
    const char *fn = "fine_windows";
    if (!d) return set_error(NOF_EINVAL, "%s: desc is NULL", fn);
    if (int rc = fm_indices(fn, d->M, d->P, d->pair, d->i, d->j)) return rc;
    if (d->N_a < 1) return set_error(NOF_EINVAL, "%s: N_a=%d must be at least 1", fn, d->N_a);
    if (d->N_b < 1) return set_error(NOF_EINVAL, "%s: N_b=%d must be at least 1", fn, d->N_b);
    if (d->stride < 1) return set_error(NOF_EINVAL, "%s: stride=%d must be at least 1", fn, d->stride);
    const struct { int32_t v; const char *name; } dims[] = {{d->h0, "h0"}, {d->w0, "w0"}, {d->h1, "h1"}, {d->w1, "w1"}};
    for (const auto &g : dims) {
        if (g.v < 1) return set_error(NOF_EINVAL, "%s: %s=%d must be at least 1", fn, g.name, g.v);
        if ((int64_t)g.v * d->stride > FM_MAX_SIDE)
            return set_error(NOF_EINVAL, "%s: stride %s=%lld must be at most %d", fn, g.name, (long long)g.v * d->stride,
                             FM_MAX_SIDE);
    }
    if (int rc = require_workspace(fn, d->weights_bytes, fm_weight_bytes(), "weights_bytes")) return rc;
    const NamedPointer ptrs[] = {
        {d->fine_a, "fine_a"}, {d->fine_b, "fine_b"}, {d->coarse_a, "coarse_a"}, {d->coarse_b, "coarse_b"},
        {d->weights, "weights"}, {d->context, "context"}, {d->win_a, "win_a"}, {d->win_b, "win_b"}};
    for (const NamedPointer &a : ptrs) {   // each pointer's alignment is judged before the next one's presence
        if (int rc = require_pointers(fn, {a})) return rc;
        if ((uintptr_t)a.p & 15) return set_error(NOF_EINVAL, "%s: %s must be 16-byte aligned", fn, a.name);
    }
    if (d->M == 0) return NOF_OK;

    const char *w = static_cast<const char *>(d->weights);
    FmArgs a{};
    a.fine[0] = (const _Float16 *)d->fine_a; a.fine[1] = (const _Float16 *)d->fine_b;
    a.coarse[0] = d->coarse_a; a.coarse[1] = d->coarse_b;
    a.frames[0] = d->frames_a; a.frames[1] = d->frames_b;
    a.pair = d->pair; a.cell[0] = d->i; a.cell[1] = d->j;
    a.M = d->M; a.P = d->P;
    a.N[0] = d->N_a; a.N[1] = d->N_b;
    a.h[0] = d->h0; a.w[0] = d->w0; a.h[1] = d->h1; a.w[1] = d->w1;
    a.stride = d->stride;
    a.w_down = (const h8v *)w;
    a.w_fine = (const h8v *)(w + (size_t)FM_C * FM_CC * 2);
    a.w_ctx = (const h8v *)(w + (size_t)FM_C * FM_CC * 2 + (size_t)FM_C * FM_C * 2);
    a.b_down = (const float *)(w + (size_t)2 * FM_C * FM_CC * 2);
    a.b_merge = a.b_down + FM_C;
    a.ctx = d->context; a.win[0] = d->win_a; a.win[1] = d->win_b;

    hipStream_t s = (hipStream_t)stream;
    const uint32_t rows = 2 * (uint32_t)d->M;
    hipLaunchKernelGGL(k_fine_context, dim3(div_up(rows, FM_CTX_ROWS)), dim3(FM_THREADS), 0, s, a);
    const uint32_t blocks = div_up(rows, 4);
    hipLaunchKernelGGL(k_fine_windows, dim3(blocks < FM_MAX_BLOCKS ? blocks : FM_MAX_BLOCKS), dim3(FM_THREADS), 0, s, a);
    return check_launch(fn);
}

int nof_fine_expectation(const nof_fine_expectation_desc *d, void *stream) {
    const char *fn = "fine_expectation";
    if (!d) return set_error(NOF_EINVAL, "%s: desc is NULL", fn);
    if (int rc = fm_indices(fn, d->M, d->P, d->pair, d->i, d->j)) return rc;
    if (d->L < 1) return set_error(NOF_EINVAL, "%s: L=%d must be at least 1", fn, d->L);
    if (d->S < 1) return set_error(NOF_EINVAL, "%s: S=%d must be at least 1", fn, d->S);
    if (int rc = require_pointers(fn, {{d->win_a, "win_a"}, {d->win_b, "win_b"}, {d->expec, "expec"}})) return rc;
    if (((uintptr_t)d->win_a | (uintptr_t)d->win_b) & 15)
        return set_error(NOF_EINVAL, "%s: win_a and win_b must be 16-byte aligned", fn);
    if (d->M == 0) return NOF_OK;
    FeArgs a{d->win_a, d->win_b, d->pair, d->i, d->j, d->M, d->P, d->L, d->S, d->expec};
    hipLaunchKernelGGL(k_fine_expect, dim3(div_up((uint32_t)d->M, 4)), dim3(FM_THREADS), 0, (hipStream_t)stream, a);
    return check_launch(fn);
}

}  // extern "C"
