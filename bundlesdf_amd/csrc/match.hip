// Descriptor matching (include/nof.h group 11): the weight-free matching head of the reference's
// LoFTR (BundleTrack/LoFTR/src/loftr/utils/coarse_matching.py, CoarseMatching.forward with
// dual_softmax and get_coarse_match) as one fused pipeline. The reference materialises the [P,L,S]
// similarity, two softmaxes and their product; here no [L,S] array exists: the 32x32 tiles of the
// similarity live in MFMA accumulators and only O(P (L + S)) statistics touch memory.
//
// Definition. For P pairs, desc_a [P,L,C] and desc_b [P,S,C] in float16, grids (h0,w0) and (h1,w1)
// with L = h0 w0 and S = h1 w1, optional cell masks valid_a [P,L] and valid_b [P,S] (uint8):
//
//   sim(i,j)  = (sum_k a_ik b_jk) * 1/(C temperature). The products of fp16 values are accumulated
//               in float32 by the MFMA; the scale (one float32 number) is applied once to the sum.
//               sim is -inf where valid_a[i] or valid_b[j] is 0.
//   conf(i,j) = exp(sim - rowmax_i) / rowsum_i * exp(sim - colmax_j) / colsum_j in float32, the row
//               statistics over j, the column statistics over i: rowmax_i = max_j sim(i,j), rowsum_i
//               = sum_j exp(sim(i,j) - rowmax_i). A row or column with no valid partner has rowmax
//               -inf, rowsum 0 and conf 0 everywhere (the reference yields NaN there).
//   (i,j) is a match iff conf(i,j) > thr, neither cell lies within border_rm cells of its grid's
//               edge, j is the lowest index attaining the maximum of row i and i is the lowest index
//               attaining the maximum of column j (the reference's == keeps every tied entry).
//
// Evaluation order (what makes two runs give the same bytes). The kernels divide by a sum by
// multiplying with its float32 reciprocal, formed once per row and column: conf = (exp(sim -
// rowmax) (1/rowsum)) * (exp(sim - colmax) (1/colsum)), the same two factors in both passes of
// k_match_best, so a pair's confidence has the same bits seen from its row and from its column.
//
//  k_match_stats  "queries" on the lanes, "keys" in the accumulator registers: a wave owns 32
//                 queries whose descriptor fragments stay in registers, a block of four waves stages
//                 tiles of 32 keys in LDS (rows padded, mfma_tile.h) and every
//                 wave multiplies the tile against its queries, C/16 MFMAs of 32x32x16 per tile. A
//                 lane then holds sim of ONE query against 16 keys and keeps that query's running
//                 maximum and running sum of exp(sim - max) without any cross-lane step; the two
//                 lane halves (the other 16 keys of every tile) meet once at the end, half 0 first.
//                 Queries = A gives the row statistics, queries = B the column statistics.
//  k_match_best   the same tiles again: conf from both sets of statistics, per query the best
//                 (conf, lowest key). Queries = A gives j of every row, queries = B i of every column.
//  k_match_emit   one block per pair: threshold, border, mutual check, the count of matches.
//
// Tails: a query or key row past L or S is staged as zeros and masked to -inf, a k-chunk past C is
// staged as zeros (C is a multiple of 8, the chunk of one lane); there is no scalar path. No
// floating-point atomics, no reduction whose order depends on scheduling.
#include "mfma_tile.h"
#include "host_entry.h"

#pragma clang fp contract(off)

namespace nof {

constexpr int MATCH_WAVES = 4;                       // waves of a block: 128 queries
constexpr int MATCH_QB = 32 * MATCH_WAVES;
constexpr int MATCH_KT = 32;                         // keys per staged tile: one MFMA tile

struct MatchSide {
    const _Float16 *q;       // [P,nq,C] queries
    const _Float16 *k;       // [P,nk,C] keys
    const uint8_t *valid_q;  // [P,nq] or null
    const uint8_t *valid_k;  // [P,nk] or null
    int nq, nk, C;
    float scale;             // 1 / (C temperature)
    // statistics: written by k_match_stats for the queries; read by k_match_best for both sides
    float *q_max, *q_sum;    // [P,nq]
    const float *k_max, *k_sum;   // [P,nk] (k_match_best only)
    int32_t *best_idx;       // [P,nq] (k_match_best only)
    float *best_conf;        // [P,nq] or null
};

// KS = 16-wide k-steps held (C <= 16 KS). BEST = false: statistics; true: best partner.
template <int KS, bool BEST>
__global__ void __launch_bounds__(64 * MATCH_WAVES) k_match_tiles(const MatchSide a) {
    constexpr int ROW_BYTES = KS * 32 + ROW_PAD;     // a staged key row: 16 KS halves plus the pad
    constexpr int CHUNKS = KS * 2;                   // 16-byte chunks of a row
    __shared__ __attribute__((aligned(16))) unsigned char tile[MATCH_KT * ROW_BYTES];
    __shared__ float key_max[MATCH_KT], key_rinv[MATCH_KT];
    __shared__ unsigned char key_ok[MATCH_KT];

    const int p = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int query = blockIdx.x * MATCH_QB + wave * 32 + r;
    const bool q_in = query < a.nq;
    const size_t qrow = (size_t)p * a.nq + (q_in ? query : 0);
    const bool q_ok = q_in && (a.valid_q == nullptr || a.valid_q[qrow] != 0);

    // the queries' fragments: lane (r, h) holds Q[query r][16 s + 8 h .. + 7] for every k-step s
    h8v qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int k0 = 16 * s + 8 * h;
        h8v v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (q_in && k0 < a.C) v = *reinterpret_cast<const h8v *>(a.q + qrow * a.C + k0);
        qf[s] = v;
    }

    float run_max = -INFINITY, run_sum = 0.f;        // statistics
    float q_max = -INFINITY, q_rinv = 0.f;           // best partner: the query's own statistics
    float best = -1.f;
    int best_idx = -1;
    if (BEST) {
        const float qs = q_in ? a.q_sum[qrow] : 0.f;
        q_max = q_in ? a.q_max[qrow] : -INFINITY;
        q_rinv = (q_ok && qs > 0.f) ? 1.0f / qs : 0.f;
    }

    const int n_tiles = (a.nk + MATCH_KT - 1) / MATCH_KT;
    for (int t = 0; t < n_tiles; ++t) {
        const int key0 = t * MATCH_KT;
        __syncthreads();                             // the previous tile has been read by every wave
        for (int idx = threadIdx.x; idx < MATCH_KT * CHUNKS; idx += 64 * MATCH_WAVES) {
            const int row = idx / CHUNKS, ch = idx % CHUNKS;
            h8v v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (key0 + row < a.nk && ch * 8 < a.C)
                v = *reinterpret_cast<const h8v *>(a.k + ((size_t)p * a.nk + key0 + row) * a.C + ch * 8);
            *reinterpret_cast<h8v *>(tile + row * ROW_BYTES + ch * 16) = v;
        }
        if (threadIdx.x < MATCH_KT) {
            const int key = key0 + threadIdx.x;
            const bool in = key < a.nk;
            const size_t krow = (size_t)p * a.nk + (in ? key : 0);
            bool ok = in && (a.valid_k == nullptr || a.valid_k[krow] != 0);
            if (BEST) {
                const float ks = in ? a.k_sum[krow] : 0.f;
                ok = ok && ks > 0.f;
                key_max[threadIdx.x] = in ? a.k_max[krow] : -INFINITY;
                key_rinv[threadIdx.x] = ok ? 1.0f / ks : 0.f;
            }
            key_ok[threadIdx.x] = ok ? 1 : 0;
        }
        __syncthreads();

        f16v acc;
        acc_zero(acc);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            // A operand: lane (r, h) holds K[key r][16 s + 8 h .. + 7]; the result has the key on the
            // register axis and the query on the lane
            mma(acc, lds_operand(tile, r, ROW_BYTES, s, h), qf[s]);
        }

        if (!BEST) {
            float v[16];
            float tmax = -INFINITY;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const bool ok = q_ok && key_ok[acc_row(q, h)] != 0;
                v[q] = ok ? acc[q] * a.scale : -INFINITY;
                tmax = fmaxf(tmax, v[q]);
            }
            const float m = fmaxf(run_max, tmax);
            if (m > -INFINITY) {
                float s = run_sum * expf(run_max - m);
#pragma unroll
                for (int q = 0; q < 16; ++q) s += expf(v[q] - m);
                run_sum = s;
                run_max = m;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = acc_row(q, h);
                if (key0 + row < a.nk) {
                    const float v = acc[q] * a.scale;
                    const float kr = key_rinv[row];
                    float conf = 0.f;
                    if (kr > 0.f && q_rinv > 0.f) conf = (expf(v - q_max) * q_rinv) * (expf(v - key_max[row]) * kr);
                    if (conf > best) {
                        best = conf;
                        best_idx = key0 + row;
                    }
                }
            }
        }
    }

    // the two lane halves hold the other 16 keys of every tile: they meet here, half 0 first
    if (!BEST) {
        const float om = __shfl_xor(run_max, 32), os = __shfl_xor(run_sum, 32);
        const float m0 = h ? om : run_max, s0 = h ? os : run_sum, m1 = h ? run_max : om, s1 = h ? run_sum : os;
        const float m = fmaxf(m0, m1);
        float s = 0.f;
        if (m > -INFINITY) s = s0 * expf(m0 - m) + s1 * expf(m1 - m);
        if (q_in && h == 0) {
            a.q_max[qrow] = m;
            a.q_sum[qrow] = s;
        }
    } else {
        const float oc = __shfl_xor(best, 32);
        const int oi = __shfl_xor(best_idx, 32);
        if (oc > best || (oc == best && oi < best_idx)) {
            best = oc;
            best_idx = oi;
        }
        if (q_in && h == 0) {
            a.best_idx[qrow] = best_idx;
            if (a.best_conf) a.best_conf[qrow] = best;
        }
    }
}

__device__ __forceinline__ bool match_inside(int cell, int w, int hgt, int b) {
    const int x = cell % w, y = cell / w;
    return x >= b && x < w - b && y >= b && y < hgt - b;
}

__global__ void __launch_bounds__(256) k_match_emit(const int32_t *row_best, const float *row_conf, const int32_t *col_best,
                                                    int L, int S, int h0, int w0, int h1, int w1, int border, float thr,
                                                    int32_t *j_of_i, float *conf, int32_t *n_matches) {
    __shared__ int32_t wave_count[4];
    const int p = blockIdx.x;
    int32_t mine = 0;
    for (int i = threadIdx.x; i < L; i += 256) {
        const size_t row = (size_t)p * L + i;
        const int j = row_best[row];
        const float c = row_conf[row];
        const bool hit = j >= 0 && j < S && c > thr && col_best[(size_t)p * S + j] == i && match_inside(i, w0, h0, border) &&
                         match_inside(j, w1, h1, border);
        j_of_i[row] = hit ? j : -1;
        conf[row] = hit ? c : 0.f;
        mine += hit ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) n_matches[p] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
}

struct MatchWs : Carver {
    float *row_max, *row_sum, *col_max, *col_sum, *row_conf;
    int32_t *row_best, *col_best;
    MatchWs(void *base, int32_t P, int32_t L, int32_t S) : Carver(base) {
        const size_t nl = (size_t)P * L, ns = (size_t)P * S;
        row_max = take<float>(nl); row_sum = take<float>(nl);
        col_max = take<float>(ns); col_sum = take<float>(ns);
        row_conf = take<float>(nl); row_best = take<int32_t>(nl);
        col_best = take<int32_t>(ns);
    }
};

template <bool BEST>
static void match_launch(const MatchSide &side, int P, hipStream_t s) {
    const dim3 grid(div_up(side.nq, MATCH_QB), (unsigned)P), block(64 * MATCH_WAVES);
    if (side.C <= 64) hipLaunchKernelGGL((k_match_tiles<4, BEST>), grid, block, 0, s, side);
    else if (side.C <= 256) hipLaunchKernelGGL((k_match_tiles<16, BEST>), grid, block, 0, s, side);
    else hipLaunchKernelGGL((k_match_tiles<32, BEST>), grid, block, 0, s, side);
}

}  // namespace nof

using namespace nof;

extern "C" {

size_t nof_match_workspace_bytes(int32_t P, int32_t L, int32_t S) {
    if (P < 1 || L < 1 || S < 1) return 0;
    return MatchWs(nullptr, P, L, S).bytes;
}

int nof_match_descriptors(const nof_match_desc *d, void *stream) {
    const char *fn = "match_descriptors";
    if (!d) return set_error(NOF_EINVAL, "%s: desc is NULL", fn);
    if (d->P < 1 || d->P > 65535) return set_error(NOF_EINVAL, "%s: P=%d must be in 1..65535", fn, d->P);
    if (d->C < 8 || d->C > 512 || d->C % 8)
        return set_error(NOF_EINVAL, "%s: C=%d must be a multiple of 8 in 8..512", fn, d->C);
    if (d->h0 < 1 || d->w0 < 1 || d->L < 1 || (int64_t)d->h0 * d->w0 != d->L)
        return set_error(NOF_EINVAL, "%s: L=%d must be h0 w0 = %d x %d, at least 1", fn, d->L, d->h0, d->w0);
    if (d->h1 < 1 || d->w1 < 1 || d->S < 1 || (int64_t)d->h1 * d->w1 != d->S)
        return set_error(NOF_EINVAL, "%s: S=%d must be h1 w1 = %d x %d, at least 1", fn, d->S, d->h1, d->w1);
    if ((int64_t)d->P * d->L >= (1ll << 31) || (int64_t)d->P * d->S >= (1ll << 31))
        return set_error(NOF_EINVAL, "%s: P L and P S must be below 2^31 (P=%d L=%d S=%d)", fn, d->P, d->L, d->S);
    if (!(d->temperature > 0.f) || !(d->temperature <= 3.0e38f))
        return set_error(NOF_EINVAL, "%s: temperature=%g must be positive and finite", fn, (double)d->temperature);
    if (!(d->thr >= 0.f && d->thr < 1.f)) return set_error(NOF_EINVAL, "%s: thr=%g must be in [0,1)", fn, (double)d->thr);
    if (d->border_rm < 0) return set_error(NOF_EINVAL, "%s: border_rm=%d must not be negative", fn, d->border_rm);
    if ((d->valid_a == nullptr) != (d->valid_b == nullptr))
        return set_error(NOF_EINVAL, "%s: %s is NULL while the other side's mask is given", fn,
                         d->valid_a ? "valid_b" : "valid_a");
    if (int rc = require_pointers(fn, {{d->desc_a, "desc_a"}, {d->desc_b, "desc_b"}, {d->workspace, "workspace"},
                                       {d->j_of_i, "j_of_i"}, {d->conf, "conf"}, {d->n_matches, "n_matches"}}))
        return rc;
    if (((uintptr_t)d->desc_a | (uintptr_t)d->desc_b) & 15)
        return set_error(NOF_EINVAL, "%s: desc_a and desc_b must be 16-byte aligned", fn);
    MatchWs ws(d->workspace, d->P, d->L, d->S);
    if (int rc = require_workspace(fn, d->workspace_bytes, ws.bytes)) return rc;

    hipStream_t s = (hipStream_t)stream;
    if (d->row_max) ws.row_max = d->row_max;
    if (d->row_sum) ws.row_sum = d->row_sum;
    if (d->col_max) ws.col_max = d->col_max;
    if (d->col_sum) ws.col_sum = d->col_sum;

    MatchSide rows{};
    rows.q = (const _Float16 *)d->desc_a; rows.k = (const _Float16 *)d->desc_b;
    rows.valid_q = d->valid_a; rows.valid_k = d->valid_b;
    rows.nq = d->L; rows.nk = d->S; rows.C = d->C;
    rows.scale = 1.0f / ((float)d->C * d->temperature);
    rows.q_max = ws.row_max; rows.q_sum = ws.row_sum; rows.k_max = ws.col_max; rows.k_sum = ws.col_sum;
    rows.best_idx = ws.row_best; rows.best_conf = ws.row_conf;
    MatchSide cols = rows;
    cols.q = rows.k; cols.k = rows.q; cols.valid_q = rows.valid_k; cols.valid_k = rows.valid_q;
    cols.nq = d->S; cols.nk = d->L;
    cols.q_max = ws.col_max; cols.q_sum = ws.col_sum; cols.k_max = ws.row_max; cols.k_sum = ws.row_sum;
    cols.best_idx = ws.col_best; cols.best_conf = nullptr;

    match_launch<false>(rows, d->P, s);
    match_launch<false>(cols, d->P, s);
    match_launch<true>(rows, d->P, s);
    match_launch<true>(cols, d->P, s);
    hipLaunchKernelGGL(k_match_emit, dim3((unsigned)d->P), dim3(256), 0, s, ws.row_best, ws.row_conf, ws.col_best, d->L,
                       d->S, d->h0, d->w0, d->h1, d->w1, d->border_rm, d->thr, d->j_of_i, d->conf, d->n_matches);
    return check_launch(fn);
}

}  // extern "C"
