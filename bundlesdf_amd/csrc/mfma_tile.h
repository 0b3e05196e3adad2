// The v_mfma_f32_32x32x16_f16 tile conventions every MFMA kernel of the library shares: the vector
// types, the lane / register layout, operand reads, staging, the tile GEMM and the fp16 rounding of an epilogue.
// Device functions and types only, no kernel.
//
// D[32,32] += A[32,16] B[16,32]^T per instruction, fp16 operands, float32 accumulation; one wave.
// With lane = 32 h + r (r = lane & 31 the row, h = lane >> 5 the lane half):
//
//  Operand fragment (h8v), the same for A and B: lane (r, h) holds row r of its matrix, k-elements
//      16 ks + 8 h .. + 7 of k-step ks. A's rows become the rows of D, B's rows its columns.
//  Accumulator (f16v): register 4 g + e (g = 0..3, e = 0..3) of lane (r, h) holds D[8 g + 4 h + e][r]:
//      A's rows lie on the registers (acc_row), B's rows on the lanes. Four consecutive registers are
//      four consecutive rows, so an epilogue moves them as one h4v / float4.
//  Fragment order of a packed matrix W [N,K] (out, in): [N/32][K/16][64][8] fp16 where entry
//      (nt, ks, lane, j) is W[32 nt + (lane & 31)][16 ks + 8 (lane >> 5) + j]: the operand of tile nt
//      and k-step ks is fragment (nt KS + ks) 64 + lane (packed_operand), and a wave reads it as 1 KB
//      of consecutive bytes. The same fragment serves as A or as B.
//  Row pad of an LDS tile: rows of 2 K bytes plus ROW_PAD = 16. A lane half reads an operand as 16
//      bytes from each of 32 rows; with the bare stride (a multiple of 128 bytes, half the 64 banks
//      of 4 bytes) those reads would fall on the same few banks, and the pad moves consecutive rows
//      four banks apart.
#pragma once
#include "nof_device.h"

namespace nof {

typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef _Float16 h4v __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int ROW_PAD = 16;

// tile row of accumulator register q in lane half h
__device__ __forceinline__ int acc_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }
__device__ __forceinline__ void acc_zero(f16v &acc) {
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
}
__device__ __forceinline__ void mma(f16v &acc, const h8v &a, const h8v &b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
}

// lane (row, h)'s operand of k-step ks from an LDS tile with rows of row_bytes
__device__ __forceinline__ h8v lds_operand(const unsigned char *tile, int row, int row_bytes, int ks, int h) {
    return *reinterpret_cast<const h8v *>(tile + row * row_bytes + ks * 32 + h * 16);
}
// this lane's operand of tile nt, k-step ks of a matrix in fragment order with KS k-steps (the index
// in int: a packed matrix here has far fewer than 2^31 fragments)
__device__ __forceinline__ h8v packed_operand(const h8v *__restrict__ w, int nt, int KS, int ks, int lane) {
    return w[(nt * KS + ks) * 64 + lane];
}

// registers 4 g .. 4 g + 3 of acc (rows acc_row(4 g, h) .. + 3) through f(value, e), rounded to fp16
template <typename F>
__device__ __forceinline__ h4v acc_quad(const f16v &acc, int g, F f) {
    h4v o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (_Float16)f(acc[4 * g + e], e);
    return o;
}

// rows row0 .. row0 + ROWS - 1 of base [n,C] float32 as fp16 into an LDS tile; zeros past n. THREADS =
// the block's size.
template <int C, int ROWS, int THREADS>
__device__ __forceinline__ void stage_rows(const float *base, int row0, int n, unsigned char *dst, int row_bytes) {
    constexpr int Q4 = C / 4;
    for (int idx = threadIdx.x; idx < ROWS * Q4; idx += THREADS) {
        const int row = idx / Q4, c4 = idx % Q4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + row < n) v = *reinterpret_cast<const float4 *>(base + (size_t)(row0 + row) * C + c4 * 4);
        const h4v o = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
        *reinterpret_cast<h4v *>(dst + row * row_bytes + c4 * 8) = o;
    }
}

// The 64 rows (two halves of 32) of the LDS tile xs against NT tiles of 32 rows of a packed W with KS
// k-steps, from its tile nt0; acc starts at zero. XS_ON_REGS: acc[i][t] has the rows of half t of xs on
// the registers and the rows of tile nt0 + i of W on the lanes; otherwise W's on the registers and xs's
// on the lanes.
template <int NT, int KS, bool XS_ON_REGS>
__device__ __forceinline__ void tile_gemm(const h8v *__restrict__ wp, int nt0, const unsigned char *xs, int row_bytes,
                                          int lane, f16v (&acc)[NT][2]) {
    constexpr int HALVES = 2;
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int t = 0; t < HALVES; ++t) acc_zero(acc[i][t]);
#pragma unroll 8
    for (int ks = 0; ks < KS; ++ks) {
        h8v w[NT], x[HALVES];
#pragma unroll
        for (int i = 0; i < NT; ++i) w[i] = packed_operand(wp, nt0 + i, KS, ks, lane);
#pragma unroll
        for (int t = 0; t < HALVES; ++t) x[t] = lds_operand(xs, 32 * t + r, row_bytes, ks, h);
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int t = 0; t < HALVES; ++t) {
                if constexpr (XS_ON_REGS) mma(acc[i][t], x[t], w[i]);
                else mma(acc[i][t], w[i], x[t]);
            }
    }
}

}  // namespace nof
