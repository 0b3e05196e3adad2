// Fused NeRF training step for gfx950 (CDNA4): ray setup + octree ray trace,
// stratified/around-depth sampling, multires grid encode, tiny MLP on MFMA,
// depth-guided compositing, SDF/free-space/colour losses and the complete
// backward pass (MLP weights, hash-table scatter, input gradient -> per-ray
// pose gradient). Replaces the per-step body of NerfRunner.train_loop
// (nerf_runner.py:677-762) — render_rays :1013-1128, the samplers
// :979-1010/:67-87, run_network :1226-1303, raw2outputs :1131-1168,
// get_sdf_loss nerf_helpers.py:382-399 and autograd.
//
// The training step only: its kernels, the scatter machinery, its host entry points. What it shares with
// the inference side (field_infer.hip) is field_core.h (device) and field_host.h (host).
//
// Work decomposition, one stream, no host synchronisation:
//  * k_trace: one lane per ray — DDA through the occupancy grid, intervals
//    converted to z, clipped at depth+trunc, summed.
//  * k_encode: one wave per (ray, 32-sample tile): z, validity, multires
//    encode; lane (sample n = l & 31, half h = l >> 5) handles levels
//    {8s + 4(q>>1) + 2h + (q&1)} — the row set of its MFMA accumulator
//    registers, so the encoding is the layer-1 B operand in place: the sigma
//    net runs on the tile, then the sdf-loss terms, the backward / colour flags
//    and the per-sample loss terms of backward tiles (tile aux).
//  * k_compact: lists of the flagged tiles (backward, colour).
//  * k_colour: persistent waves over the colour tiles (colour net on MFMA);
//    k_ray_final: a thread per ray — compositing and losses.
//  * k_mlp_bwd: two persistent passes over the list: the tile's forward is
//    recomputed, the MFMA backward runs, every weight / bias gradient is
//    accumulated in registers over the wave's tiles (one atomic per element at
//    the end); dL/dfeature, the SH part of the pose gradient. amp:
//    k_mlp_bwd_tr takes the weight gradients' K = samples operands from LDS
//    transposes (mlp_lds.h) instead of swapped-operand recomputes. Both live in
//    field_mlp_bwd.h, included in place below (training only).
//  * k_scatter: one wave per ray: the ray's backward samples compacted, corner
//    re-gather, input gradient, table gradient reduced in registers (DPP) and
//    LDS before one HBM atomic per distinct row; the point part of the pose
//    gradient.
#include <array>
#include <vector>

#include "field_core.h"
#include "field_host.h"

#pragma clang fp contract(off)

namespace nof {

constexpr int LOSS_ACC_COUNTERS = 136;
constexpr int LOSS_ACC_WORDS = 144;   // loss_acc's length (include/nof.h)
// per tile (tile-parallel forward): the tile's partial sums, stored (not added) by k_encode SIG
// (weight sum, valid count, sdf terms, work-counter bits: every in-range tile) and k_colour
// (composited colour, fs_rgb term: colour tiles only); k_ray_final sums a ray's tiles in tile
// order, so the ray's sums are deterministic (raw2outputs' fixed-order sum) — no float atomics
constexpr int TREC = 12;
enum { TR_WSUM = 0, TR_NVALID, TR_LFS, TR_LEM, TR_LSDF, TR_CNT, TR_RACC = 8, TR_LFSR = 11 };
enum { TC_SIG = 1, TC_COL = 2, TC_CRCOL = 4, TC_CRSIG = 8 };   // TR_CNT bits (as an int)
constexpr int LOSS_COPIES = 64, LOSS_SLOTS = 16, LOSS_FOLD_N = 13;
// workspace words zeroed per step: the record counter (+ padding to 16 words) and the loss rows
constexpr uint64_t LOSS_ZERO_WORDS = 16 + (uint64_t)LOSS_COPIES * LOSS_SLOTS;

// DPP helpers: value of lane n+d (row_shl) / n-d (row_shr) inside the 16-lane
// row, 0 outside it.
template <int CTRL> __device__ __forceinline__ int dpp_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}
#define DPP_ROW_SHL(n) (0x100 + (n))
#define DPP_ROW_SHR(n) (0x110 + (n))

// Backward of one level (kernel_grid_backward + kernel_input_backward,
// gridencoder.cu:249-365) for this lane's sample: adds d<g, feature>/d x01
// (the reference's dy_dx, re-gathered, never materialised) to gx and
// accumulates w*g of the 8 corners into the wave's LDS hash table.
//
// MI355X: device float atomics cost one memory-side request per active lane
// (~20 G lane-ops/s chip-wide, same-address lanes are NOT merged), so the
// scatter is reduced twice before it reaches HBM: (1) the lanes hold
// consecutive samples of one ray, so equal cells form contiguous runs — a
// segmented suffix sum over each 16-lane DPP row folds a run into its head;
// (2) heads insert into a per-wave open-addressing table in LDS keyed by the
// global table row, which dedupes across rows, chunks and corner slots for
// the whole ray at this level. flush_table then issues one HBM atomic per
// distinct row. MUST be called by all lanes of the wave (DPP).
constexpr uint32_t SLOT_EMPTY = 0xffffffffu;

// relaxed, wave-local LDS CAS: lets the 8 corner claims of a lane stay in flight together
__device__ __forceinline__ uint32_t lds_cas(uint32_t *p, uint32_t key) {
    uint32_t e = SLOT_EMPTY;
    __hip_atomic_compare_exchange_strong(p, &e, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return e;   // previous content
}

// LDS row table of one scatter wave. amp (F16V): interleaved slots [key | packed fp16x2 value]
// (8 B; the claim and the add use one address), fp32: keys[mask + 1] then float2 values.
template <bool F16V> __device__ __forceinline__ uint32_t *slot_key(uint32_t *keys, uint32_t s) {
    return keys + (F16V ? 2 * s : s);
}
__device__ __forceinline__ void lds_add_h2(void *vals, uint32_t s, uint32_t packed) {
    // one packed fp16x2 LDS add (the reference's __half2 accumulation class); vals = keys + 1
    __builtin_amdgcn_ds_atomic_fadd_v2f16(
        (__attribute__((address_space(3))) h2v *)(reinterpret_cast<uint32_t *>(vals) + 2 * s),
        __builtin_bit_cast(h2v, packed));
}
template <bool F16V>
__device__ __forceinline__ void lds_add(void *vals, uint32_t s, float v0, float v1) {
    if constexpr (F16V) {
        lds_add_h2(vals, s, __builtin_bit_cast(uint32_t, h2v{(_Float16)v0, (_Float16)v1}));
    } else {
        float *f = reinterpret_cast<float *>(vals) + 2 * s;
        __hip_atomic_fetch_add(f, v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(f + 1, v1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// Slow path of a claim whose home slot holds another row: linear probing from
// the next slot; a full probe chain goes straight to HBM (returns false).
template <bool F16V>
__device__ __forceinline__ bool lds_probe(uint32_t *keys, void *vals, uint32_t mask, uint32_t key, float v0, float v1,
                                          float *g32, __half *g16) {
    uint32_t s = key;
#pragma unroll 1
    for (int p = 1; p < 16; ++p) {
        s = (s + 1) & mask;
        const uint32_t old = lds_cas(slot_key<F16V>(keys, s), key);
        if (old == SLOT_EMPTY || old == key) {
            lds_add<F16V>(vals, s, v0, v1);
            return true;
        }
    }
    if (g16) atomic_add_h2(g16 + (size_t)key * 2, v0, v1);
    else { atomic_add_f32(g32 + (size_t)key * 2, v0); atomic_add_f32(g32 + (size_t)key * 2 + 1, v1); }
    return false;
}

// amp form of gather_level for the input gradient: the corner pairs stay fp16x2 and are
// contracted with g = (g0, g1) by one v_dot2_f32_f16 each (fp32 accumulation of the exact
// fp16 products): t[k] = g0 e[k][0] + g1 e[k][1], without converting the 16 corner values
__device__ __forceinline__ void gather_level_t16(const FieldArgs &a, const LevelInfo &li, h2v g01, float t[8],
                                                 const uint32_t rows[8]) {
    const __half *tab = reinterpret_cast<const __half *>(a.table);
    const uint32_t rs = li.res + 1;
    if (level_dense(rs, li.hs)) {
#pragma unroll
        for (int idx = 0; idx < 8; idx += 2) {   // dense: corners idx, idx+1 are adjacent rows
            uint2 v;
            __builtin_memcpy(&v, tab + (size_t)rows[idx] * 2, 8);
            t[idx] = __builtin_amdgcn_fdot2(__builtin_bit_cast(h2v, v.x), g01, 0.f, false);
            t[idx + 1] = __builtin_amdgcn_fdot2(__builtin_bit_cast(h2v, v.y), g01, 0.f, false);
        }
    } else {
#pragma unroll
        for (int idx = 0; idx < 8; ++idx) {
            const uint32_t v = *reinterpret_cast<const uint32_t *>(tab + (size_t)rows[idx] * 2);
            t[idx] = __builtin_amdgcn_fdot2(__builtin_bit_cast(h2v, v), g01, 0.f, false);
        }
    }
}

// member: the lane holds one of the ray's compacted backward samples (its cell takes part in the runs);
// active: its dL/dfeature at this level is non-zero (its terms are non-zero). part: 1 for the
// around-depth samples, 0 for the octree samples (see the run keys below)
template <typename TT, bool F16V>
__device__ __forceinline__ void backward_level(const FieldArgs &a, const LevelInfo &li, bool member, bool active,
                                               uint32_t part, const float x01[3], float g0, float g1, h2v g01,
                                               float gx[3], int lane, uint32_t *keys, void *vals, uint32_t mask,
                                               float *g32, __half *g16, int &n_direct) {
    // every lane's cell, weights and rows, unconditionally (a member's sample is in the box: pos >= 0.5,
    // truncation = floor; a non-member lane computes finite values it never uses — a branch here only
    // made the compiler materialise zeros for the skipped lanes)
    float pos[3];
    uint32_t pg[3], crow[8];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        pos[d] = __builtin_fmaf(x01[d], li.scale, 0.5f);
        pg[d] = (uint32_t)pos[d];
        pos[d] = __builtin_amdgcn_fractf(pos[d]);
    }
    corner_rows(li, pg, crow);
    if (active && !a.no_dx) {   // frozen poses: no corner values
        // d<g, feature>/d x01 of the trilinear interpolant (the reference's dy_dx contracted
        // with g): one scalar field t = g0 e[.][0] + g1 e[.][1] over the 8 corners, then its
        // x / y / z slopes by successive lerps (bit d of the corner index = +1 along d)
        float t[8];
        if constexpr (sizeof(TT) == 2) {
            gather_level_t16(a, li, g01, t, crow);
        } else {
            float e[8][2], pos_unused[3];
            uint32_t rows_unused[8];
            gather_level<TT, true>(a, li, x01, pos_unused, e, rows_unused);
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = __builtin_fmaf(g1, e[k][1], g0 * e[k][0]);
        }
        float dx[4], ax[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {            // j = y + 2 z
            dx[j] = t[2 * j + 1] - t[2 * j];
            ax[j] = __builtin_fmaf(pos[0], dx[j], t[2 * j]);
        }
        float dy[2], by[2], ux[2];
#pragma unroll
        for (int z = 0; z < 2; ++z) {
            dy[z] = ax[2 * z + 1] - ax[2 * z];
            by[z] = __builtin_fmaf(pos[1], dy[z], ax[2 * z]);
            ux[z] = __builtin_fmaf(pos[1], dx[2 * z + 1] - dx[2 * z], dx[2 * z]);
        }
        gx[0] = __builtin_fmaf(li.scale, __builtin_fmaf(pos[2], ux[1] - ux[0], ux[0]), gx[0]);
        gx[1] = __builtin_fmaf(li.scale, __builtin_fmaf(pos[2], dy[1] - dy[0], dy[0]), gx[1]);
        gx[2] = __builtin_fmaf(li.scale, by[1] - by[0], gx[2]);
    }
    if ABL(1) return;
    // run keys: exact cell coordinates (10 bits each; res <= 1023) and the sample part in bit 31;
    // lanes past the ray's list unique. Within a part the samples are in ascending z, so a straight ray
    // visits each cell in one contiguous stretch: equal keys are always one run (the around-depth part
    // revisits the octree part's cells, hence the part bit), and a member whose dL/dfeature is zero
    // keeps its cell's key with zero terms, so it never splits a run
    const int key = member ? (int)((1u + (pg[0] | (pg[1] << 10) | (pg[2] << 20))) | (part << 31))
                           : (0x40000000 + lane + 1);
    // One representative per run of the whole wave: the run's TAIL (last lane), after a
    // segmented inclusive prefix sum across the wave (row_shr 1..8 inside each 16-lane row,
    // then row_bcast:15 / row_bcast:31 carry row totals into the next rows for runs that
    // cross a row boundary). Heads-per-row (a suffix scan inside rows) made a run that
    // crosses rows claim the same 8 slots once per row, in the same LDS instruction.
    // wave_shr:1 / wave_shl:1 (GFX9 DPP): the neighbour lanes' keys across row boundaries;
    // lanes 0 / 63 read 0, which is never a key
    const bool tail = member && (dpp_i<0x130>(key) != key);
    if (ABL(1 << 27)) {   // timing-build probe: representatives (tails)
        n_direct += tail ? 1 : 0;
    }
    // s_d: the lane's run continues d lanes back inside its row (in-row sources before the row start
    // read 0, never a key); equal keys are one run, so no run ids are needed
    const bool s1 = dpp_i<DPP_ROW_SHR(1)>(key) == key, s2 = dpp_i<DPP_ROW_SHR(2)>(key) == key;
    const bool s4 = dpp_i<DPP_ROW_SHR(4)>(key) == key, s8 = dpp_i<DPP_ROW_SHR(8)>(key) == key;
    // cross-row steps: the lane's run includes the row_bcast:15 source (lane 15 / 47, rows 1 / 3) or
    // the row_bcast:31 source (lane 31, rows 2 / 3)
    const bool sb15 = __builtin_amdgcn_update_dpp(0, key, 0x142, 0xa, 0xf, false) == key;
    const bool sb31 = __builtin_amdgcn_update_dpp(0, key, 0x143, 0xc, 0xf, false) == key;
    // wave-uniform: the scan steps some run actually needs (s_d: run continues d lanes back)
    const bool any1 = __any(s1), any2 = __any(s2);
    const bool any4 = __any(s4), any8 = __any(s8);
    const bool anyb15 = __any(sb15), anyb31 = __any(sb31);
    // corner weights times g (inactive lanes: g = 0 and pos = 0, so every value is 0)
    const float h0 = active ? g0 : 0.f, h1 = active ? g1 : 0.f;
    float wxy[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wxy[j] = ((j & 1) ? pos[0] : 1 - pos[0]) * ((j & 2) ? pos[1] : 1 - pos[1]);
    const float wz0[2] = {(1 - pos[2]) * h0, pos[2] * h0}, wz1[2] = {(1 - pos[2]) * h1, pos[2] * h1};
    float v0[8], v1[8];
#pragma unroll
    for (int idx = 0; idx < 8; ++idx) {
        v0[idx] = wxy[idx & 3] * wz0[idx >> 2];
        v1[idx] = wxy[idx & 3] * wz1[idx >> 2];
    }
    // segmented prefix sum (runs are contiguous): one wave-uniform branch per scan step and
    // one v_fmac_f32_dpp per value: v += v[src] * m with m in {0, 1} (exactly v + x or v;
    // in-row sources before the row start read 0). Written as asm because the compiler
    // splits the DPP read from the FMA.
    // amp (F16V): the 16 values are packed into 8 fp16 pairs first (the LDS table holds fp16
    // pairs anyway) and scanned by v_pk_fmac_f16 with DPP — half the scan instructions. A run's
    // terms are then summed in fp16 (a tree of log2(run) roundings), the rounding class of the
    // reference, which adds every sample-corner term into the fp16 gradient one by one
    // (gridencoder.cu:319-327). Timing build: ABL 4096 keeps the fp32 scan.
    uint32_t pk[8];
    const bool pscan = F16V && !ABL(4096);
    if (pscan) {
#pragma unroll
        for (int idx = 0; idx < 8; ++idx) pk[idx] = __builtin_bit_cast(uint32_t, h2v{(_Float16)v0[idx], (_Float16)v1[idx]});
#define PFMAC_DPP(I, CTRL) "v_pk_fmac_f16_dpp %" #I ", %" #I ", %8 " CTRL "\n"
#define PSCAN_STEP(SK, CTRL)                                                                                      \
        if (any##SK) {                                                                                            \
            const uint32_t m = s##SK ? 0x3C003C00u : 0u;                                                          \
            asm("s_nop 1\n" PFMAC_DPP(0, CTRL) PFMAC_DPP(1, CTRL) PFMAC_DPP(2, CTRL) PFMAC_DPP(3, CTRL)          \
                PFMAC_DPP(4, CTRL) PFMAC_DPP(5, CTRL) PFMAC_DPP(6, CTRL) PFMAC_DPP(7, CTRL)                      \
                : "+v"(pk[0]), "+v"(pk[1]), "+v"(pk[2]), "+v"(pk[3]), "+v"(pk[4]), "+v"(pk[5]), "+v"(pk[6]),     \
                  "+v"(pk[7])                                                                                     \
                : "v"(m));                                                                                        \
        }
        PSCAN_STEP(1, "row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        PSCAN_STEP(2, "row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        PSCAN_STEP(4, "row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        PSCAN_STEP(8, "row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1")
        PSCAN_STEP(b15, "row_bcast:15 row_mask:0xa bank_mask:0xf")
        PSCAN_STEP(b31, "row_bcast:31 row_mask:0xc bank_mask:0xf")
#undef PFMAC_DPP
#undef PSCAN_STEP
    }
#define FMAC_DPP(I, CTRL) "v_fmac_f32_dpp %" #I ", %" #I ", %16 " CTRL "\n"
#define SCAN_STEP(SK, CTRL)                                                                                       \
    if (!pscan && any##SK) {                                                                                      \
        const float m = s##SK ? 1.f : 0.f;                                                                        \
        asm("s_nop 1\n" FMAC_DPP(0, CTRL) FMAC_DPP(1, CTRL) FMAC_DPP(2, CTRL) FMAC_DPP(3, CTRL)                  \
            FMAC_DPP(4, CTRL) FMAC_DPP(5, CTRL) FMAC_DPP(6, CTRL) FMAC_DPP(7, CTRL) FMAC_DPP(8, CTRL)            \
            FMAC_DPP(9, CTRL) FMAC_DPP(10, CTRL) FMAC_DPP(11, CTRL) FMAC_DPP(12, CTRL) FMAC_DPP(13, CTRL)        \
            FMAC_DPP(14, CTRL) FMAC_DPP(15, CTRL)                                                                \
            : "+v"(v0[0]), "+v"(v0[1]), "+v"(v0[2]), "+v"(v0[3]), "+v"(v0[4]), "+v"(v0[5]), "+v"(v0[6]),         \
              "+v"(v0[7]), "+v"(v1[0]), "+v"(v1[1]), "+v"(v1[2]), "+v"(v1[3]), "+v"(v1[4]), "+v"(v1[5]),         \
              "+v"(v1[6]), "+v"(v1[7])                                                                            \
            : "v"(m));                                                                                            \
    }
    SCAN_STEP(1, "row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1")
    SCAN_STEP(2, "row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1")
    SCAN_STEP(4, "row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1")
    SCAN_STEP(8, "row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1")
    SCAN_STEP(b15, "row_bcast:15 row_mask:0xa bank_mask:0xf")
    SCAN_STEP(b31, "row_bcast:31 row_mask:0xc bank_mask:0xf")
#undef FMAC_DPP
#undef SCAN_STEP
    if (!tail) return;
    if (ABL(1 << 26)) {   // timing build: the DPP scan without the table claims / adds
        n_direct += (v0[0] + v1[7] == 12345.f || (pscan && pk[3] == 12345u)) ? 1 : 0;
        return;
    }
    if constexpr (F16V) {
        if (!pscan) {   // the fp32 scan's sums, packed once (v_cvt_pk_f16_f32)
#pragma unroll
            for (int idx = 0; idx < 8; ++idx)
                pk[idx] = __builtin_bit_cast(uint32_t, h2v{(_Float16)v0[idx], (_Float16)v1[idx]});
        }
    }
    // claim the 8 home slots (home = the row itself mod the table size: the x-runs of
    // corner rows stay in consecutive slots, so the in-order flush issues few 64-B
    // segments per instruction) with all 8 CASes in flight, then add
    uint32_t old[8];
#pragma unroll
    for (int idx = 0; idx < 8; ++idx) old[idx] = lds_cas(slot_key<F16V>(keys, crow[idx] & mask), crow[idx]);
    // adds without branches: a claim that lost its home slot adds 0 there (harmless) and
    // takes the probe path afterwards, in one wave-uniform branch that is rarely entered
    // (which claims lost is recomputed there from old[])
    bool all_ok = true;
#pragma unroll
    for (int idx = 0; idx < 8; ++idx) {
        const bool ok = old[idx] == SLOT_EMPTY || old[idx] == crow[idx];
        all_ok = all_ok && ok;
        if constexpr (F16V) {   // the packed sums, selected once
            lds_add_h2(vals, crow[idx] & mask, ok ? pk[idx] : 0u);
        } else {
            lds_add<F16V>(vals, crow[idx] & mask, ok ? v0[idx] : 0.f, ok ? v1[idx] : 0.f);
        }
    }
    if (__builtin_expect(__any(!all_ok), 0)) {
#pragma unroll
        for (int idx = 0; idx < 8; ++idx)
            if (!(old[idx] == SLOT_EMPTY || old[idx] == crow[idx])) {
                float u0 = v0[idx], u1 = v1[idx];
                if constexpr (F16V) {   // the scanned fp16 pair (exact in fp32)
                    const h2v q = __builtin_bit_cast(h2v, pk[idx]);
                    u0 = (float)q[0];
                    u1 = (float)q[1];
                }
                n_direct += lds_probe<F16V>(keys, vals, mask, crow[idx], u0, u1, g32, g16) ? 0 : 1;
            }
    }
}

// One HBM atomic per occupied slot, then the slot is emptied for the next level.
// Lane l takes slots l + 64 j (consecutive lanes -> consecutive home slots -> rows
// in few 64-B segments per atomic instruction); four slots per lane are read
// together, every slot is reset unconditionally, so each group of 256 slots costs
// one LDS round trip instead of one per occupied slot.
// NJ (compile-time) slots per lane of one group of 64 NJ slots: the reads are issued together (a
// run-time slot count per group made the compiler wait after each read), the resets, then the adds
template <bool F16V, int NJ>
__device__ __forceinline__ int flush_group(uint32_t *keys, void *vals, uint32_t s0, int lane, float *g32, __half *g16,
                                           bool no_hbm) {
    uint32_t k[NJ];
    uint32_t vb[NJ];          // F16V: packed fp16x2
    float va[NJ], vc[NJ];     // fp32 pairs
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const uint32_t sl = s0 + 64 * j + lane;
        if constexpr (F16V) {   // [key | value] in one 8-B read
            const uint2 kv = reinterpret_cast<const uint2 *>(keys)[sl];
            k[j] = kv.x;
            vb[j] = kv.y;
        } else {
            k[j] = keys[sl];
            const float2 v = reinterpret_cast<float2 *>(vals)[sl];
            va[j] = v.x; vc[j] = v.y;
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const uint32_t sl = s0 + 64 * j + lane;
        if constexpr (F16V) {
            reinterpret_cast<uint2 *>(keys)[sl] = make_uint2(0xffffffffu, 0u);
        } else {
            keys[sl] = 0xffffffffu;
            reinterpret_cast<float2 *>(vals)[sl] = make_float2(0.f, 0.f);
        }
    }
    int n = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        n += (int)__popcll(__ballot(k[j] != 0xffffffffu));   // wave-uniform count (scalar register)
        if (k[j] != 0xffffffffu && !no_hbm) {
            if constexpr (F16V) {
                typedef _Float16 h2v __attribute__((ext_vector_type(2)));
                __builtin_amdgcn_global_atomic_fadd_v2f16((__attribute__((address_space(1))) h2v *)(g16 + (size_t)k[j] * 2),
                                                          __builtin_bit_cast(h2v, vb[j]));
            } else if (g16) {
                atomic_add_h2(g16 + (size_t)k[j] * 2, va[j], vc[j]);
            } else {
                atomic_add_f32(g32 + (size_t)k[j] * 2, va[j]);
                atomic_add_f32(g32 + (size_t)k[j] * 2 + 1, vc[j]);
            }
        }
    }
    return n;
}
template <bool F16V>
__device__ __forceinline__ int flush_table(uint32_t *keys, void *vals, uint32_t mask, int lane, float *g32,
                                           __half *g16, bool no_hbm) {
    int n = 0;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (mask + 1 >= 256) {   // 256 .. 2048 slots: groups of four slots per lane
        for (uint32_t s0 = 0; s0 <= mask; s0 += 256) n += flush_group<F16V, 4>(keys, vals, s0, lane, g32, g16, no_hbm);
    } else if (mask + 1 == 128) {
        n = flush_group<F16V, 2>(keys, vals, 0, lane, g32, g16, no_hbm);
    } else {
        n = flush_group<F16V, 1>(keys, vals, 0, lane, g32, g16, no_hbm);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    return n;
}

__global__ __launch_bounds__(256) void k_ray_ctx(FieldArgs a_) {
    const FieldArgs a = step_args(a_);
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    // the step's counters, loss rows and loss_acc are zeroed here (one launch fewer per step; the
    // step is a captured graph of kernel nodes only)
    for (int i = r; i < (int)LOSS_ZERO_WORDS; i += gridDim.x * blockDim.x) a.n_tiles[i] = 0;
    for (int i = r; i < LOSS_ACC_WORDS; i += gridDim.x * blockDim.x) a.loss_acc[i] = 0.f;
    if (r >= a.R) return;
    const RayCtx c = build_ray(a, r);
    store_ray_ctx(a.rctx, r, c);
}

// Feature / feature-gradient rows are stored per sample in MFMA-fragment
// order: 4 chunks of 8 elements, chunk (s*2 + h) = the B-operand fragment of
// K step s for lane half h. One lane's chunk = 16 B (fp16) / 32 B (fp32).
template <typename TM>
__device__ __forceinline__ void store_chunk(void *buf, size_t sample0, int n, int s, int h, const typename FragT<TM>::T &f) {
    // sample0 (the tile's first sample) is wave-uniform: a scalar 64-bit base plus a 32-bit lane offset
    TM *p = reinterpret_cast<TM *>(buf) + sample0 * 32 + (uint32_t)(n * 32 + (s * 2 + h) * 8);
    if constexpr (sizeof(TM) == 2) {
        *reinterpret_cast<h8v *>(p) = f;
    } else {
        *reinterpret_cast<float4 *>(p) = make_float4(f.v[0], f.v[1], f.v[2], f.v[3]);
        *reinterpret_cast<float4 *>(p + 4) = make_float4(f.v[4], f.v[5], f.v[6], f.v[7]);
    }
}
// dL/dfeature, level-major: plane lv holds the (feature 0, feature 1) pair of every
// sample ([L][R*S][2] TM), so k_scatter's per-level read is one coalesced 256-B (fp16)
// row per wave instead of 64 lanes each touching their own 64-B sample row. The
// fragment chunk (ss, h) holds levels lane_level(ss, q, h), q = 0..3 (2 values each).
template <typename TM>
__device__ __forceinline__ void store_dfeat(void *buf, size_t RS, size_t sample0, int n, int ss, int h,
                                            const typename FragT<TM>::T &f) {
    // the plane bases of the lane half's levels are wave-uniform (sample0 = the tile's first sample; h
    // selects between two uniform bases): scalar 64-bit arithmetic, a 32-bit lane offset
    TM *p = reinterpret_cast<TM *>(buf) + sample0 * 2;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int l0 = 8 * ss + 4 * (q >> 1) + (q & 1);
        TM *d0 = p + (size_t)l0 * RS * 2, *d1 = p + (size_t)(l0 + 2) * RS * 2;
        TM *d = (h ? d1 : d0) + (uint32_t)(n * 2);
        if constexpr (sizeof(TM) == 2) {
            typedef _Float16 h2v __attribute__((ext_vector_type(2)));
            h2v v = {f[2 * q], f[2 * q + 1]};
            *reinterpret_cast<h2v *>(d) = v;
        } else {
            *reinterpret_cast<float2 *>(d) = make_float2(f.v[2 * q], f.v[2 * q + 1]);
        }
    }
}
template <typename TM>
__device__ __forceinline__ typename FragT<TM>::T load_chunk(const void *buf, size_t sample0, int n, int s, int h) {
    const TM *p = reinterpret_cast<const TM *>(buf) + sample0 * 32 + (uint32_t)(n * 32 + (s * 2 + h) * 8);
    typename FragT<TM>::T f;
    if constexpr (sizeof(TM) == 2) {
        f = *reinterpret_cast<const h8v *>(p);
    } else {
        const float4 u = *reinterpret_cast<const float4 *>(p), v = *reinterpret_cast<const float4 *>(p + 4);
        f.v[0] = u.x; f.v[1] = u.y; f.v[2] = u.z; f.v[3] = u.w; f.v[4] = v.x; f.v[5] = v.y; f.v[6] = v.z; f.v[7] = v.w;
    }
    return f;
}

// per ray: [0..2] dL/drgb (x rgb_weight, ray weight, 1/3R), [3] wtot, [4] ray weight
constexpr int RAY_AUX = 8;

// per flagged tile (float4): [lane] (fp32 k_mlp_bwd pass 0 -> pass 1) ReLU masks of H3, H3^t, H4;
// [64 + n] (sdf-loss gradient without the ray weight, depth-guided weight if valid, valid, fs_rgb
// front) of sample n; [96 + n] (fp32 pass 0 -> pass 1) dO of sample n; [128 ..] (k_encode -> k_colour /
// pass 0) the colour-net input fragment Cin[0] of the tile (16 B per lane fp16 at [128 + lane], 32 B
// fp32 at [128 + 2 lane]), overwritten by amp pass 0 with the sigma-net output gradient for pass 1
// (fp16, [128 + lane]); amp only (k_colour -> k_mlp_bwd_tr pass 0): the SH fragment Cin[1] at
// [192 + lane], the ray's view directions in .zw of [0..2] (vd0 vd1 | vd2 R vd.x | R vd.y R vd.z)
constexpr int TILE_AUX = 256;
template <typename TM>
__device__ __forceinline__ void store_cin(float4 *aux, int lane, const typename FragT<TM>::T &f) {
    if constexpr (sizeof(TM) == 2) {
        reinterpret_cast<h8v *>(aux + 128)[lane] = f;
    } else {
        aux[128 + 2 * lane] = make_float4(f.v[0], f.v[1], f.v[2], f.v[3]);
        aux[129 + 2 * lane] = make_float4(f.v[4], f.v[5], f.v[6], f.v[7]);
    }
}
template <typename TM>
__device__ __forceinline__ typename FragT<TM>::T load_cin(const float4 *aux, int lane) {
    typename FragT<TM>::T f;
    if constexpr (sizeof(TM) == 2) {
        f = reinterpret_cast<const h8v *>(aux + 128)[lane];
    } else {
        const float4 u = aux[128 + 2 * lane], v = aux[129 + 2 * lane];
        f.v[0] = u.x; f.v[1] = u.y; f.v[2] = u.z; f.v[3] = u.w; f.v[4] = v.x; f.v[5] = v.y; f.v[6] = v.z; f.v[7] = v.w;
    }
    return f;
}
// loss_acc layout: [0..7] loss terms / counts, [8..135] spread scatter atomic counters,
// [136..139] forward executed-work counters (sigma tiles, colour tiles, colour records, sigma records),
// [140] fs_rgb loss (normalised, unscaled; cfg fs_rgb_weight > 0)

// The kernels' per-wave loss terms and work counters go to LOSS_COPIES copies of a 16-slot row
// (copy = wave id mod LOSS_COPIES) and loss_fold (first wave of the scatter kernel) adds the copies into loss_acc at the end of the
// field pass: one HBM atomic per wave and slot on a single address serialises at the memory side
// (the former per-ray forward's 13 per-wave loss atomics from 4096 persistent waves cost 0.09 ms per step).
// Slots: 0..4 loss rgb / fs / empty / sdf / n_valid, 5 n_bwd, 6..9 work counters, 10 fs_rgb loss,
// 11..12 timing-build probes; LOSS_FOLD_DST = their loss_acc indices.

__device__ __forceinline__ float *loss_row(const FieldArgs &a, int wave_id) {
    return a.loss_part + (size_t)(wave_id & (LOSS_COPIES - 1)) * LOSS_SLOTS;
}

// amp: the ReLU-derivative factors of a 64-row activation kept per pair (0 / 1 per half, the v_pk_min_u16
// result relu_mask packs into bits) for a mask consumed within the same tile, and its packed bits
__device__ __forceinline__ uint32_t relu_factors(const h8v (&H)[2][2], uint32_t (&r)[16]) {
    uint32_t m = 0;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int P = 8 * t + 4 * s + p;
                r[P] = pair_bits(h2v{H[t][s][2 * p], H[t][s][2 * p + 1]}, 0);
                m |= r[P] << P;
            }
    return m;
}
// masked_frags with the factors of relu_factors: one packed multiply per pair
__device__ __forceinline__ void masked_frags_r(const f16v (&acc)[2], const uint32_t (&r)[16], h8v (&d)[2][2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const uint32_t u = __builtin_bit_cast(uint32_t, pk_round(acc[t][8 * s + 2 * p], acc[t][8 * s + 2 * p + 1]));
                uint32_t v;
                asm("v_pk_mul_lo_u16 %0, %1, %2" : "=v"(v) : "v"(u), "v"(r[8 * t + 4 * s + p]));
                frag_put2(d[t][s], p, __builtin_bit_cast(h2v, v));
            }
}

// ------------------------------------------------------ kernel 1: encode + sigma net
// One wave per (ray, 32-sample tile): stratified/around-depth z
// (render_rays :1060-1080), world point, validity, and the multires
// encoding of the lane's 8 levels (kernel_grid, gridencoder.cu:106-246) —
// the lane layout is the layer-1 MFMA B operand, so the sigma net runs on the
// tile in place. Low register count -> high occupancy for the latency-bound
// gathers. SGPRs capped at 80: on gfx950 a wave's SGPR block (count rounded up to 16, + 16) comes
// out of an 800-entry budget per SIMD, so the 95 the compiler wanted admitted 7 waves per SIMD —
// 3 of these 8-wave blocks per CU, 6 waves per SIMD — where 80 admit 8 (MI355X_MICROARCH.md,
// residency); amp: 64 VGPRs (8 waves per SIMD), the uniform values spill to VGPR lanes
// DBG: the debug outputs (dbg_z / dbg_valid / dbg_raw) are written; the production instance compiles
// them out (their pointers and branches took SGPRs the 80-SGPR cap then spilled to VGPR lanes)
template <typename TM, typename TT, int G, bool DBG>
__global__ __launch_bounds__(512) __attribute__((amdgpu_num_sgpr(80),
                                                 amdgpu_waves_per_eu(sizeof(TM) == 2 ? (G == 1 ? 8 : G == 2 ? 6 : 4) : (G == 4 ? 4 : 5), 8)))
void k_encode(FieldArgs a_) {
    const FieldArgs a = step_args(a_);
    const int lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
    const int ntiles = a.S / 32;
    constexpr int WPB = 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    {
        // layer 1 / 2 weight fragments (FR_L1, FR_L2: 8 x 1 KB fp16) and their biases, copied global -> LDS
        // by LDS-DMA (global_load_lds: no registers, no wait here): one 16-B piece per lane and fp16 KB,
        // the biases by the first two waves; the block's barrier comes after the gathers
        typedef __attribute__((address_space(1))) void *GPtr;
        typedef __attribute__((address_space(3))) void *LPtr;
        const int wv = threadIdx.x >> 6;
        if (ABL(16)) {   // timing build: synchronous staging through registers, barrier before the gathers
            const uint4 *src = reinterpret_cast<const uint4 *>(a.frags);
            uint4 *dst = reinterpret_cast<uint4 *>(smem);
            for (int i = threadIdx.x; i < 8 * 64 * 8 * (int)sizeof(TM) / 16; i += blockDim.x) dst[i] = src[i];
            float *s_b = reinterpret_cast<float *>(smem + 8 * 64 * 8 * sizeof(TM));
            for (int i = threadIdx.x; i < 2 * 64; i += blockDim.x) s_b[i] = a.bias[i];
            __syncthreads();
        } else {
#pragma unroll
            for (int i = 0; i < (int)sizeof(TM) / 2; ++i) {
                const size_t off = (size_t)i * 8192 + (size_t)wv * 1024;
                __builtin_amdgcn_global_load_lds((GPtr)((const char *)a.frags + off + lane * 16), (LPtr)(smem + off), 16,
                                                 0, 0);
            }
            if (wv < 2)
                __builtin_amdgcn_global_load_lds((GPtr)(a.bias + wv * 64 + lane),
                                                 (LPtr)(smem + 8 * 64 * 8 * sizeof(TM) + wv * 256), 4, 0, 0);
        }
    }
    // the wave's level table (after the weights and biases): the encode reads each lane's level record from it
    uint4 *lvt = reinterpret_cast<uint4 *>(smem + 8 * 64 * 8 * sizeof(TM) + 2 * 64 * sizeof(float)) + (threadIdx.x >> 6) * 32;
    level_table(a, lvt, lane);
    const int bx = (a.xcd_order & 1) ? xcd_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int gw0 = __builtin_amdgcn_readfirstlane(bx * WPB + (int)(threadIdx.x >> 6));
    const bool in_range = gw0 < a.R * ntiles;
    // every wave reaches the block barrier; a wave past the last tile encodes the last tile
    // again (no stores) and leaves after it
    const int gw = in_range ? gw0 : a.R * ntiles - 1;
    const int r = gw / ntiles, t = gw - r * ntiles;
    if (ABL(1 << 19)) return;   // timing build: the waves' launch, staging and nothing else
    const RayCtx c = load_ray(a, r);
    const int s = 32 * t + n;
    const size_t sid = (size_t)r * a.S + s;
    float z = sample_z(a, r, s, c.depth, c.vdepth, c.total, c.box);
    if (ABL(4)) {   // timing build: the sampler's interval walk twice (its cost = the difference)
        const float z2 = sample_z(a, r, s, c.depth * 0.999f, c.vdepth, c.total * 0.999f, c.box);
        z = z2 == 12345.f ? z2 : z;
    }
    float p[3], x[3];
    const bool valid = sample_point(c, z, p, x);
    if (h == 0 && in_range) {
        a.zbuf[sid] = z;
        if (DBG && a.dbg_z) a.dbg_z[sid] = z;
        if (DBG && a.dbg_valid) a.dbg_valid[sid] = valid;
    }
    if (ABL(8192)) return;   // timing build: the sampler and the z store only
    const float x01[3] = {(x[0] + 1) / 2, (x[1] + 1) / 2, (x[2] + 1) / 2};
    typename FragT<TM>::T f[2];
#pragma unroll
    for (int g0 = 0; g0 < 8; g0 += G) {
        int lvs[G];
#pragma unroll
        for (int k = 0; k < G; ++k) lvs[k] = lane_level((g0 + k) >> 2, (g0 + k) & 3, h);
        float v[G][2];
        encode_levels<TT, G, true, true>(a, lvs, valid && !ABL(8), x01, v, lvt);
#pragma unroll
        for (int k = 0; k < G; ++k) {
            frag_set<TM>(f[(g0 + k) >> 2], 2 * ((g0 + k) & 3), v[k][0]);
            frag_set<TM>(f[(g0 + k) >> 2], 2 * ((g0 + k) & 3) + 1, v[k][1]);
        }
    }
    {
        // the sigma net on the tile just encoded (the features are the layer-1 B operand as they
        // stand), and everything of the forward tile pass that needs only the sdf: loss terms, the
        // backward / colour flags, the per-sample loss terms and gradient mask of backward tiles,
        // the colour-net input of colour tiles; features are stored only for backward tiles
        if (!ABL(64)) __syncthreads();   // the staged fragments (timing build: ABL 64 skips the barrier)
        if (!in_range) return;
        // the tail's arguments (loss weights, output pointers) re-read from the kernel arguments here,
        // after the gathers, instead of held in SGPRs across them (the 80-SGPR cap spilled them)
        const FieldArgs a = step_args(late_args());
        const bool tvalid = __any(valid);
        uint8_t *flag = a.tile_bwd + (size_t)r * ntiles + t;
        float4 *trec = reinterpret_cast<float4 *>(a.rrec + ((size_t)r * ntiles + t) * TREC);
        // the tile's share of the ray's weight sum (every sample, raw2outputs) and valid count in ONE
        // reduction: both lane halves hold the tile's 32 samples, the lower half carries the weight,
        // the upper half the valid flag (timing build: ABL 2 skips the per-tile record's reductions)
        float ws = 0.f, nv = 0.f;
        if (!ABL(2)) half_sums(h == 0 ? bell_weight(a, c.depth, z) : (valid ? 1.f : 0.f), ws, nv);
        if (!tvalid && !(DBG && a.dbg_raw)) {
            if (lane == 0) {
                *flag = 0;
                if (trec) {
                    trec[0] = make_float4(ws, nv, 0.f, 0.f);
                    trec[1] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            return;
        }
        const TM *s_fr = reinterpret_cast<const TM *>(smem);
        const float *s_b = reinterpret_cast<const float *>(smem + 8 * 64 * 8 * sizeof(TM));
        Acts<TM> A;
        A.X[0] = f[0];
        A.X[1] = f[1];
        float sdf = 0.f;
        f16v l2;
        if (ABL(256)) {   // timing build: no sigma-net MFMAs
#pragma unroll
            for (int q = 0; q < 16; ++q) l2[q] = 0.f;
            sdf = z * 1e-3f;
        } else {
            mlp_sdf_net<TM>(LdsWt<TM>(s_fr, lane), s_b, A, lane, sdf, l2);   // one tile per wave: no fence needed
        }
        const float w = bell_weight(a, c.depth, z);
        const bool front = z < c.depth - a.trunc;
        const bool fsr = a.fs_rgb_w > 0.f && front && valid && c.rtype == 0;
        const bool colour = __any(w > 0.f && valid) || __any(fsr) || (DBG && a.dbg_raw != nullptr);
        const float sv = valid ? 1.f : 0.f;
        const bool back = z > c.depth + a.trunc * a.ntr;
        const float sdfm = (!front && !back && c.vdepth) ? 1.f : 0.f;
        const bool fsm = (c.depth > a.far_sc) && (sdf < a.fs_sdf);
        const bool em = front && (c.depth <= a.far_sc) && (sdf < 1.f);
        const float efs = fsm ? (sdf - a.fs_sdf) : 0.f;
        const float esdf = (z + sdf * a.trunc) * sdfm - c.depth * sdfm;
        float dsdf = a.fs_w * 0.5f * 2.f * efs * sv * a.inv_RS;
        dsdf += em ? a.fs_w * a.empty_w * (sdf > 1.f ? 1.f : (sdf < 1.f ? -1.f : 0.f)) * sv * a.inv_RS : 0.f;
        dsdf += a.trunc_w * 0.5f * 2.f * esdf * sdfm * a.trunc * sv * a.inv_RS;
        const bool cand = tvalid && c.rtype == 0 && (__any(w > 0.f && valid) || __any(dsdf != 0.f) || __any(fsr));
        // 1: backward with the colour net, 2: sigma-only backward, 3: colour net in the forward only
        if (lane == 0) *flag = cand ? (colour ? 1 : 2) : (colour ? 3 : 0);
        if (trec && !ABL(2)) {   // the tile's sdf-loss terms (ray weight applied by k_ray_final) and work-counter bits
            // a sample's fs / empty / sdf terms are mutually exclusive (depth > far / front / the band),
            // so a tile whose every loss gradient dsdf is zero has zero loss values too: no reductions.
            // Otherwise two reductions: fs (lower half) with empty (upper half), then sdf
            float lfs = 0.f, lem = 0.f, lsd = 0.f;
            if (__any(dsdf != 0.f)) {
                half_sums(h == 0 ? a.fs_w * 0.5f * efs * efs * sv * a.inv_RS
                                 : (em ? a.fs_w * a.empty_w * fabsf(sdf - 1.f) * sv * a.inv_RS : 0.f),
                          lfs, lem);
                float unused;
                half_sums(h == 0 ? a.trunc_w * 0.5f * esdf * esdf * sv * a.inv_RS : 0.f, lsd, unused);
            }
            if (lane == 0) {
                const int cnt = TC_SIG | (colour ? TC_COL : 0) | (cand ? (colour ? TC_CRCOL : TC_CRSIG) : 0);
                trec[0] = make_float4(ws, nv, lfs, lem);
                trec[1] = make_float4(lsd, __int_as_float(cnt), 0.f, 0.f);
            }
            // (the sample id re-derived from the tile's scalar slot: keeping the 64-bit sid live across the
            // gathers spilled it to scratch, one 8-B store per lane and tile)
            if (DBG && a.dbg_raw && h == 0) a.dbg_raw[(((size_t)r * ntiles + t) * 32 + n) * 4 + 3] = sdf;
        }
        const size_t slot = (size_t)r * ntiles + t;
        if (ABL(32768)) return;   // timing build: no backward / colour hand-off stores
        if (cand) {
            store_chunk<TM>(a.feat, (size_t)r * a.S + 32 * t, n, 0, h, f[0]);
            store_chunk<TM>(a.feat, (size_t)r * a.S + 32 * t, n, 1, h, f[1]);
            if (h == 0) a.tile_aux[slot * TILE_AUX + 64 + n] = make_float4(dsdf, valid ? w : 0.f, sv, fsr ? 1.f : 0.f);
            const uint32_t gmask = (uint32_t)__ballot(h == 0 && valid && (w > 0.f || dsdf != 0.f || fsr));
            if (lane == 0) a.tile_gmask[slot] = gmask;
        }
        if (colour) {
            typename FragT<TM>::T cin;
            acc_to_frag<TM>(l2, 0, false, cin);
            store_cin<TM>(a.tile_aux + slot * TILE_AUX, lane, cin);
        }
    }
}

// k_colour stages the colour net's fragments only (FR_L3 .. FR_B5 - 1: 16 of the 46, 16 KB in fp16) and the
// bias image: it needs nothing else, and a third of the LDS lets more of its blocks share a CU
constexpr int COL_FR0 = FR_L3, COL_NFR = FR_B5 - FR_L3;
// the training kernels stage through this function, as they always did (in place they compile differently)
template <typename TM, int NFR, int FR0>
__device__ __forceinline__ void stage_block(const FieldArgs &a, char *smem) {
    NOF_STAGE_FRAGS(TM, NFR, FR0, false, a, smem, (staged_bias<TM, NFR>(smem)));
    __syncthreads();
}

// ---------------------------- kernel 2 (tile-parallel forward): colour net + ray finalisation
// k_encode SIG ran the sigma net, the sdf-loss terms and the flags; what is left of the forward's
// per-ray pass is the colour net on the colour tiles (flag 1 or 3, k_compact's colour list) and the
// per-ray compositing / losses. k_colour: persistent waves over the colour-tile list — a wave per
// TILE, not per ray, so independent tiles fill the SIMDs (a per-ray forward wave walked its ray's six
// tiles one after another) — colour net from the stored colour-net input, the tile's composited
// colour and fs_rgb term stored in the tile's record (rrec), and the SH fragment / view directions the
// backward reads. k_ray_final: a thread per ray — rgb_map, dL/drgb, the ray weight and the losses
// (raw2outputs + train_loop :687-751), the backward's per-ray hand-off (ray_aux), the loss rows.
template <typename TM, int WPB, int WAVES, bool DBG>
__global__ __launch_bounds__(WPB * 64) __attribute__((amdgpu_waves_per_eu(WAVES, WAVES))) void k_colour(FieldArgs a_) {
    const FieldArgs a = step_args(a_);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = lane & 31, h = lane >> 5;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    stage_block<TM, COL_NFR, COL_FR0>(a, smem);
    const float *s_b = staged_bias<TM, COL_NFR>(smem);
    LdsWt<TM> W(reinterpret_cast<const TM *>(smem), lane, COL_FR0);
    const int n_col = __builtin_amdgcn_readfirstlane(a.n_tiles[1]);
    const int wg = __builtin_amdgcn_readfirstlane((int)blockIdx.x * WPB + wave);
    const int stride = gridDim.x * WPB;
    // the tile's vector loads (colour-net input, depths, flag) are issued one tile ahead, the list
    // entry two tiles ahead: a tile starts with its inputs in flight or landed instead of one
    // memory latency (k_encode wrote them; they come from L2 / HBM) at 4 waves per SIMD
    typedef typename FragT<TM>::T Frag;
    int cur = wg < n_col ? a.ctile_list[wg] : 0;
    int nxt = a.ctile_list[min(wg + stride, max(n_col - 1, 0))];
    Frag cin_n;
    frag_zero<TM>(cin_n);
    float z_n = 0.f;
    auto fetch = [&](int sid_first) {
        z_n = a.zbuf[(size_t)sid_first + n];
        cin_n = load_cin<TM>(a.tile_aux + (size_t)(sid_first >> 5) * TILE_AUX, lane);
    };
    if (wg < n_col) fetch(__builtin_amdgcn_readfirstlane(cur));
    // the first prefetch has landed before the loop (a builtin wait the compiler tracks), so the
    // loop header's merged state does not make every tile wait on the previous tile's stores
    __builtin_amdgcn_s_waitcnt(0x0f70);
    // The loop body is straight-line in its memory operations (no store or load under a branch:
    // the per-lane stores are made wave-wide with duplicate lanes writing identical data, the debug
    // dump is a template instance): the compiler's wait counts then name exactly the load a value
    // needs. Each prefetched register is consumed where it landed before its reload is issued (no
    // loop-carried copy of an in-flight load): z at the tile's top, the colour-net input by the
    // net, after which the next tile's loads go out (the last tile re-fetches itself, clamped); the
    // list entry two tiles ahead is loaded at the top and copied at the tile's end.
    for (int li = wg; li < n_col; li += stride) {
        const int sid0 = __builtin_amdgcn_readfirstlane(cur);
        const int nn = a.ctile_list[min(li + 2 * stride, n_col - 1)];
        const int r = sid0 / a.S;
        const size_t slot = (size_t)(sid0 >> 5);
        const size_t sid = (size_t)sid0 + n;
        const RayCtx c = load_ray(a, r);
        const float z = z_n;
        const float w = bell_weight(a, c.depth, z);
        float p[3], x[3];
        const bool valid = sample_point(c, z, p, x);
        const bool front = z < c.depth - a.trunc;
        // the sample's weights, computed here (pinned: not sunk past the reload of z_n)
        float wc = valid && w > 0.f ? w : 0.f;
        float wf = a.fs_rgb_w > 0.f && front && valid && c.rtype == 0 ? a.inv_3RS : 0.f;
        asm volatile("" : "+v"(wc), "+v"(wf));
        const Frag shf = sh_frag<TM>(c, h, a.n_ff);
        Acts<TM> A;
        float logit[3];
        W.fence();   // the fragment reads stay in this tile
        mlp_colour_net_cin<TM>(W, s_b, A, cin_n, shf, lane, logit);
        fetch(__builtin_amdgcn_readfirstlane(li + stride < n_col ? nxt : sid0));
        // both lane halves hold the tile's 32 samples (the logits are broadcast): the lower half carries
        // the composited colour's r and b, the upper half g and the fs_rgb term — two half-wave sums
        // fs_rgb: mean over R x S x 3 of ((sigmoid - 1) front)^2 sw; the ray weight in k_ray_final
        float rc[3], lf = 0.f;
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            const float sg = sigmoidf(logit[cc]);
            rc[cc] = wc * sg;
            lf += (sg - 1.f) * (sg - 1.f) * wf;
        }
        if constexpr (DBG) {
            if (h == 0) {
                float *o = a.dbg_raw + sid * 4;
                o[0] = logit[0]; o[1] = logit[1]; o[2] = logit[2];
            }
        }
        if constexpr (sizeof(TM) == 2) {
            // the SH fragment and the ray's view directions for k_mlp_bwd_tr (read for backward tiles,
            // flag 1; written for every colour tile, whose aux rows hold nothing else there). The view
            // directions are three float2 words: lanes 2..63 all write word 2's identical data
            reinterpret_cast<h8v *>(a.tile_aux + slot * TILE_AUX + 192)[lane] = shf;
            float vx, vy, vz;
            view_dir(c, vx, vy, vz);
            const float2 d = lane == 0 ? make_float2(c.vd[0], c.vd[1])
                                       : (lane == 1 ? make_float2(c.vd[2], vx) : make_float2(vy, vz));
            reinterpret_cast<float2 *>(a.tile_aux + slot * TILE_AUX + min(lane, 2))[1] = d;
        }
        float s0, s1, s2, sf;
        half_sums(h == 0 ? rc[0] : rc[1], s0, s1);
        half_sums(h == 0 ? rc[2] : lf, s2, sf);
        // wave-uniform sums: every lane writes the same 16 B (no lane-0 branch)
        reinterpret_cast<float4 *>(a.rrec + slot * TREC)[2] = make_float4(s0, s1, s2, sf);
        cur = nxt;
        nxt = nn;
    }
}

__global__ __launch_bounds__(256) void k_ray_final(FieldArgs a_) {
    const FieldArgs a = step_args(a_);
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // loss rgb, fs, empty, sdf, n_valid, fs_rgb, and the four work counters
    float v[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) v[k] = 0.f;
    if (r < a.R) {
        // the ray's tiles in order: every tile's sdf record, the colour record of the colour tiles
        const int ntiles = a.S / 32;
        float wtot = 0.f, nvalid = 0.f, lfs = 0.f, lem = 0.f, lsdf = 0.f, lfsr = 0.f;
        float racc[3] = {0.f, 0.f, 0.f};
        int csig = 0, ccol = 0, crcol = 0, crsig = 0;
        // every load of a tile issued together (the colour record is read whatever the flag and
        // selected after: a flag-dependent load was a second round trip per tile)
#pragma unroll 4
        for (int t = 0; t < ntiles; ++t) {
            const size_t slot = (size_t)r * ntiles + t;
            const float4 *q = reinterpret_cast<const float4 *>(a.rrec + slot * TREC);
            const float4 q0 = q[0], q1 = q[1], q2 = q[2];
            const uint8_t fl = a.tile_bwd[slot];
            wtot += q0.x; nvalid += q0.y; lfs += q0.z; lem += q0.w; lsdf += q1.x;
            const int cnt = __float_as_int(q1.y);
            csig += cnt & TC_SIG; ccol += (cnt >> 1) & 1; crcol += (cnt >> 2) & 1; crsig += (cnt >> 3) & 1;
            if (fl == 1 || fl == 3) {
                racc[0] += q2.x; racc[1] += q2.y; racc[2] += q2.z; lfsr += q2.w;
            }
        }
        const float *cx = a.rctx + (size_t)r * RCTX;
        const float tgt[3] = {cx[3], cx[4], cx[5]};
        const int frame = __float_as_int(cx[23]), rtype = __float_as_int(cx[24]);
        const bool vray = nvalid > 0.f && rtype == 0;
        const float rw = vray ? (frame == 0 ? a.ffw : 1.f) : 0.f;
        float drgb[3], lr = 0.f, rgb[3];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            rgb[cc] = racc[cc] / (wtot + 1e-10f);
            const float e = rgb[cc] - tgt[cc];
            drgb[cc] = a.rgb_w * 2.f * e * rw * a.inv_3R;
            lr += e * e * rw;
        }
        v[0] = a.rgb_w * lr * a.inv_3R;
        v[1] = lfs * rw;
        v[2] = lem * rw;
        v[3] = lsdf * rw;
        v[4] = nvalid;
        v[5] = lfsr * rw;
        v[6] = (float)csig; v[7] = (float)ccol; v[8] = (float)crcol; v[9] = (float)crsig;
        if (a.dbg_rgb) {
            a.dbg_rgb[r * 3] = rgb[0]; a.dbg_rgb[r * 3 + 1] = rgb[1]; a.dbg_rgb[r * 3 + 2] = rgb[2];
        }
        // per-ray hand-off: dL/drgb, wtot, ray weight; the pose gradient starts at zero
        float4 *ra = reinterpret_cast<float4 *>(a.ray_aux + (size_t)r * RAY_AUX);
        ra[0] = make_float4(drgb[0], drgb[1], drgb[2], wtot);
        ra[1] = make_float4(rw, 0.f, 0.f, 0.f);
        float4 *rg = reinterpret_cast<float4 *>(a.ray_grad + (size_t)r * 12);
        rg[0] = make_float4(0.f, 0.f, 0.f, 0.f);
        rg[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        rg[2] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __shared__ float s_v[4][10];
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const float t = wave_sum(v[k]);
        if (lane == 0) s_v[wave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < 10) {
        const int k = threadIdx.x;
        const float t = s_v[0][k] + s_v[1][k] + s_v[2][k] + s_v[3][k];
        constexpr int slot[10] = {0, 1, 2, 3, 4, 10, 6, 7, 8, 9};
        if (t != 0.f && (k != 5 || a.fs_rgb_w > 0.f)) atomic_add_f32(loss_row(a, (int)blockIdx.x) + slot[k], t);
    }
}

// k_encode levels in flight per lane below 8,192 rays (FieldArgs::encode_group 0: by batch size)
constexpr int ENCODE_GROUP_SMALL = 2;

// Lists of the tiles k_encode flagged (the order inside a list is free: the MLP backward only
// sums over it). Backward tiles: those with the colour net (tile_bwd 1) from the list's FRONT,
// counted at count[0], as first sample ids; the sigma-only ones (2) from its BACK (entry j at
// n - 1 - j), counted at count[2], as first sample id | bit 31 — so the MLP backward walks the two
// kinds in separate loops with straight-line bodies (no merge of the colour path's loads with the
// other path in the loop, whose conservative wait would hold every tile on its own loads). With
// clist, in the same pass: the colour tiles (flag 1 or 3: the colour net runs in the forward,
// k_colour) as first sample ids, counted at count[1]. One returning atomic per list and block of
// 4096 flags.
constexpr int COMPACT_PER_BLOCK = 4096;   // flags per block at the headline sizes
__global__ __launch_bounds__(256) void k_compact(const uint8_t *__restrict__ flags, int n, int *__restrict__ list,
                                                 int *__restrict__ count, int per_block, int *__restrict__ clist) {
    // a thread's flags are per_block / 256 consecutive bytes (16 at 4096 per block: one 16-B
    // load), so one block-wide scan of the per-thread counts places every entry (in index order)
    __shared__ int s_wave[3][4];
    __shared__ int s_base[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int fpt = per_block >> 8;   // 16 or 2
    const int b0 = blockIdx.x * per_block + threadIdx.x * fpt;
    uint8_t fl[16];
    if (fpt == 16 && b0 + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(flags + b0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) fl[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) fl[k] = (k < fpt && b0 + k < n) ? flags[b0 + k] : 0;
    }
    // per thread: colour-backward (1), sigma-only backward (2), colour (1 or 3) counts
    int mine[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        mine[0] += fl[k] == 1;
        mine[1] += fl[k] == 2;
        mine[2] += (fl[k] == 1 || fl[k] == 3);
    }
    int pm[3] = {mine[0], mine[1], mine[2]};   // inclusive wave scans
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int u = __shfl_up(pm[q], o, 64);
            if (lane >= o) pm[q] += u;
        }
    }
    if (lane == 63) {
#pragma unroll
        for (int q = 0; q < 3; ++q) s_wave[q][wave] = pm[q];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int q = threadIdx.x;
        const int tot = s_wave[q][0] + s_wave[q][1] + s_wave[q][2] + s_wave[q][3];
        int *cnt = count + (q == 0 ? 0 : (q == 1 ? 2 : 1));
        s_base[q] = (tot && (q < 2 || clist)) ? atomicAdd(cnt, tot) : 0;
    }
    __syncthreads();
    int off[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        off[q] = s_base[q] + pm[q] - mine[q];
        for (int w = 0; w < wave; ++w) off[q] += s_wave[q][w];
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int i = b0 + k;
        if (fl[k] == 1) list[off[0]++] = i << 5;
        if (fl[k] == 2) list[n - 1 - off[1]++] = (i << 5) | (int)0x80000000;
        if (clist && (fl[k] == 1 || fl[k] == 3)) clist[off[2]++] = i << 5;
    }
}

// entry li of the backward list walked as one sequence: the colour-backward tiles [0, n_c) at the
// front, then the sigma-only tiles from the back (k_compact)
__device__ __forceinline__ int bwd_entry(const FieldArgs &a, int li, int n_c, int cap) {
    return a.tile_sid[li < n_c ? li : cap - 1 - (li - n_c)];
}

#include "field_mlp_bwd.h"   // kernel 3: the MLP backward (k_mlp_bwd, k_mlp_bwd_tr)

// The loss rows (64 copies, written by k_ray_final and k_mlp_bwd pass 1) summed into
// loss_acc: run by the first wave of the scatter kernel's first block (the scatter launches after
// every loss-row writer and writes none of these words: one launch fewer per step).
// End of the field pass: loss_acc[LOSS_FOLD_DST[k]] += sum of the LOSS_COPIES copies of slot k
__device__ __forceinline__ void loss_fold(const float *__restrict__ part, float *__restrict__ loss_acc, int k) {
    if (k >= LOSS_FOLD_N) return;
    constexpr int dst[LOSS_FOLD_N] = {0, 1, 2, 3, 4, 5, LOSS_ACC_COUNTERS, LOSS_ACC_COUNTERS + 1, LOSS_ACC_COUNTERS + 2,
                                      LOSS_ACC_COUNTERS + 3, LOSS_ACC_COUNTERS + 4, LOSS_ACC_COUNTERS + 5,
                                      LOSS_ACC_COUNTERS + 6};
    float s = 0.f;
    for (int c = 0; c < LOSS_COPIES; ++c) s += part[c * LOSS_SLOTS + k];
    loss_acc[dst[k]] += s;
}

// --------------------------------------------------- kernel 3: scatter
// LDS words of one scatter wave: the row table (keys, VW value words per slot) and the
// compacted list of the ray's backward samples (uint16, up to 320)
__host__ __device__ constexpr uint32_t scatter_wave_words(uint32_t mask, int VW) {
    return (1 + VW) * (mask + 1) + 160;
}
// One wave per ray with any tile marked by kernel 2. Levels outer, 64-sample
// chunks inner: re-gathers the corners to form d<g,feature>/dx (the
// reference's dy_dx), reduces the table gradient of the whole ray at this
// level in the wave's LDS hash table (backward_level) and flushes it with one
// HBM atomic per distinct row, and adds the transform_pts part of dL/dtf
// (sum over samples of 0.5 dL/dx01 (x) [p, 1]) to the ray's 3x4 gradient.
// SGPRs capped at 80 as k_encode's, so the hardware admits 8 waves per SIMD instead of 7 (a wave's SGPR
// block, count rounded up to 16 + 16, out of 800 per SIMD). Round 5 measured the cap neutral with 94
// SGPRs wanted (2.00 / 2.03 vs 2.02 / 2.03 ms); with the ray's pose rows re-read per iteration (92
// wanted, no spill uncapped) it measured 1.959 vs 2.001 ms uncapped and 2.033 for round 5's kernel
// (medians of 5, alternating builds, profiles/r6/ab_r6_scatter_ctx_reload_sgpr_cap.jsonl)
template <typename TM, typename TT, bool F16V, int WAVES>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80), amdgpu_waves_per_eu(WAVES, 8))) void k_scatter(FieldArgs a_) {
    const FieldArgs a = step_args(a_);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (blockIdx.x == 0 && wave == 0) loss_fold(a.loss_part, a.loss_acc, lane);
    const int bx = (a.xcd_order & 2) ? xcd_block(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    // small batches (NerfRunner.train's 2048 rays) split each ray's levels over several waves
    // so the chip has enough of them; large batches keep one wave per ray (lpw = L)
    const int lpw = a.scatter_lpw, ngrp = ((int)a.L + lpw - 1) / lpw;
    const int gw = __builtin_amdgcn_readfirstlane(bx * 4 + wave);
    const int r = __builtin_amdgcn_readfirstlane(gw / ngrp);
    if (r >= a.R || ABL(65536)) return;
    const int lv0 = __builtin_amdgcn_readfirstlane((gw - r * ngrp) * lpw);
    const int nlev = min(lpw, (int)a.L - lv0);
    const int ntiles = a.S / 32;
    const uint8_t *flags = a.tile_bwd + (size_t)r * ntiles;
    // the tiles' flags and gradient masks are loaded together (lane t: tile t; one memory latency, not two
    // dependent ones); a mask counts only for a backward tile (flag 1 / 2; 3: forward-only colour tile)
    const uint8_t fl = lane < ntiles ? flags[lane] : (uint8_t)0;
    uint32_t gm = lane < ntiles ? a.tile_gmask[(size_t)r * ntiles + lane] : 0u;
    const bool tf = fl == 1 || fl == 2;
    if (!__any(tf) || ABL(131072)) return;
    gm = tf ? gm : 0u;
    const uint32_t mask = a.slot_mask;
    constexpr int VW = F16V ? 1 : 2;   // value words per slot
    uint32_t *keys = reinterpret_cast<uint32_t *>(smem) + (size_t)wave * scatter_wave_words(mask, VW);
    // amp: interleaved [key | value] slots (vals = keys + 1, stride 2 words); fp32: keys, then values
    uint32_t *vals = F16V ? keys + 1 : keys + mask + 1;
    uint16_t *slist = reinterpret_cast<uint16_t *>(keys + (1 + VW) * (mask + 1));
    if constexpr (F16V) {
        for (uint32_t s = lane; s <= mask; s += 64) reinterpret_cast<uint2 *>(keys)[s] = make_uint2(0xffffffffu, 0u);
    } else {
        for (uint32_t s = lane; s <= mask; s += 64) keys[s] = 0xffffffffu;
        for (uint32_t s = lane; s < VW * (mask + 1); s += 64) vals[s] = 0u;
    }
    if ABL(262144) return;
    float *g32 = (sizeof(TM) == 2) ? nullptr : a.grad_table;
    __half *g16 = (sizeof(TM) == 2) ? a.grad_table16 : nullptr;
    const RayCtx c = load_ray(a, r);
    // The ray's backward samples — in a flagged tile, inside the box, and carrying a loss
    // gradient (k_encode's per-sample loss terms in the tile aux: a depth-guided weight, an
    // sdf-loss term or the fs_rgb term; every other sample's dL/dfeature is exactly zero, since
    // the rendering weights do not depend on the network) — compacted in sample order into
    // the wave's LDS list, so the (level, chunk) iterations run over full 64-lane chunks.
    // Sample order is kept, so runs of equal cells stay contiguous (two runs of one cell
    // separated by skipped samples merge: same sum).
    int n_act = 0;
    for (int ch = 0; ch * 64 < a.S; ++ch) {
        const int s = 64 * ch + lane;
        // this chunk's two tiles' masks (lanes 0-31: tile 2 ch, 32-63: tile 2 ch + 1), read from lanes 2 ch, 2 ch + 1
        const uint32_t m0 = (uint32_t)__builtin_amdgcn_readlane((int)gm, 2 * ch);
        const uint32_t m1 = 2 * ch + 1 < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)gm, 2 * ch + 1) : 0u;
        const bool cand = s < a.S && (((lane < 32 ? m0 : m1) >> (s & 31)) & 1u);
        const uint64_t b = __ballot(cand);
        if (cand) slist[n_act + (int)__popcll(b & ((1ull << lane) - 1ull))] = (uint16_t)s;
        n_act += (int)__popcll(b);
    }
    n_act = __builtin_amdgcn_readfirstlane(n_act);
    if (n_act == 0) return;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const int nch = (n_act + 63) / 64;
    // dL/dtf of the ray (transform_pts part): sum over samples of 0.5 gx (x) [p, 1] with
    // p = dir z, i.e. 0.5 (sum gx z) (x) dir and 0.5 sum gx: six per-lane sums
    float sgz[3] = {0.f, 0.f, 0.f}, sg[3] = {0.f, 0.f, 0.f};
    int n_flush = 0, n_direct = 0;   // HBM atomics issued: table flushes / probe-chain overflow
    if (!ABL(32)) {
        // (level, chunk) iterations, levels outer; the depth and the dL/dfeature pair of the
        // next iteration are loaded one iteration ahead (independent of this iteration's
        // gathers), so each iteration waits on one dependent round trip (the corner gather)
        typedef typename std::conditional<sizeof(TM) == 2, uint32_t, float2>::type GPair;
        const size_t RS = (size_t)a.R * a.S;
        const int n_it = nlev * nch;
        // unconditional loads (a lane past the list reads the ray's sample 0; the last iteration
        // re-reads a valid level): a branch around them made the compiler's wait counts conservative
        auto issue = [&](int lv, int ch, float &z, GPair &g, uint32_t &prt) {
            const int j = 64 * ch + lane;   // < 64 ceil(S / 64) <= 320: inside the list's LDS words
            const int sj_raw = (int)slist[j];
            const int sj = j < n_act ? sj_raw : 0;
            const size_t sid = (size_t)r * a.S + sj;
            prt = sj >= a.N_oct ? 1u : 0u;   // the around-depth part of the ray's samples
            z = a.zbuf[sid];
            g = reinterpret_cast<const GPair *>(a.dfeat)[(size_t)lv * RS + sid];
        };
        float z_nx = 0.f;
        GPair g_nx{};
        uint32_t prt_nx = 0u;
        issue(lv0, 0, z_nx, g_nx, prt_nx);
        // (level, chunk) of this iteration and of the next one, stepped without divisions
        int lv = lv0, ch = 0, lv_n = lv0, ch_n = 0;
        for (int it = 0; it < n_it; ++it) {
            const float z = z_nx;
            const GPair gq = g_nx;
            const uint32_t part = prt_nx;
            if (++ch_n == nch) { ch_n = 0; ++lv_n; }
            issue(min(lv_n, (int)a.L - 1), ch_n, z_nx, g_nx, prt_nx);
            const bool member = 64 * ch + lane < n_act;
            // unconditionally (a non-member lane's z, g are zero: finite values it never uses)
            float p[3], x[3], g0, g1;
            h2v g01;
            // the ray's pose rows re-read per iteration (scalar-cache hits): held across the loop they
            // took 15 SGPRs, which kept the kernel above the 80 that admit 8 waves per SIMD
            sample_point(load_ray<true>(a, r), z, p, x);   // a member's sample is inside the box (compaction)
            if constexpr (sizeof(TM) == 2) {
                g01 = __builtin_bit_cast(h2v, gq);
                g0 = (float)g01[0];
                g1 = (float)g01[1];
            } else {
                g01 = h2v{(_Float16)0.f, (_Float16)0.f};
                g0 = gq.x;
                g1 = gq.y;
            }
            const bool act = member && (g0 != 0.f || g1 != 0.f);
            if (ABL(1 << 25)) {   // utilisation probe (timing build): active lanes / busy-iteration lanes
                n_flush += __any(act) ? (int)__popcll(__ballot(act)) : 0;
                n_direct += (__any(act) && lane == 0) ? 64 : 0;
            }
            // timing build: ABL_SKIPQ skips a quarter of the levels (their gathers, scan, claims and
            // flush; the loads of the iteration stay) — the per-level-group split of the kernel time
            const bool skipq = ABL(ABL_SKIPQ(lv >> 2));
            if (__any(act) && !skipq) {
                const LevelInfo li = level_info_uniform(a, lv);   // lv is wave-uniform: a scalar load
                const float x01[3] = {(x[0] + 1) / 2, (x[1] + 1) / 2, (x[2] + 1) / 2};
                float gx[3] = {0.f, 0.f, 0.f};
                backward_level<TT, F16V>(a, li, member, act, part, x01, g0, g1, g01, gx, lane, keys, vals, mask, g32, g16,
                                         n_direct);
                // dL/dx_world = 0.5 dL/dx01 (grid.py:160)
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    sgz[i] = __builtin_fmaf(gx[i], z, sgz[i]);
                    sg[i] += gx[i];
                }
            }
            if (ch == nch - 1 && !ABL(1) && !ABL(1 << 22) && !skipq) {
                const int nfl = flush_table<F16V>(keys, vals, mask, lane, g32, g16, ABL(128));
                n_flush += nfl;
            }
            if (++ch == nch) { ch = 0; ++lv; }
        }
    }
    if (!a.no_dx) {
        float tz[3], t1[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            tz[i] = 0.5f * wave_sum(sgz[i]);
            t1[i] = 0.5f * wave_sum(sg[i]);
        }
        if (lane < 12) {
            const int i = lane >> 2, j = lane & 3;
            const float gzi = i == 0 ? tz[0] : (i == 1 ? tz[1] : tz[2]);
            const float g1i = i == 0 ? t1[0] : (i == 1 ? t1[1] : t1[2]);
            const float dj = j == 0 ? c.dir[0] : (j == 1 ? c.dir[1] : c.dir[2]);
            const float v = j < 3 ? gzi * dj : g1i;
            if (ngrp == 1) a.ray_grad[(size_t)r * 12 + lane] += v;
            else atomic_add_f32(a.ray_grad + (size_t)r * 12 + lane, v);
        }
    }
    // HBM atomic counters (diagnostics, count_atomics only: 9 us of NerfRunner.train's 0.31 ms step
    // otherwise), spread over 64 slot pairs: one hot address taking an atomic from every wave
    // serialises at the memory side (~0.45 ms per step)
    // n_flush is wave-uniform (ballot counts in flush_table), n_direct per lane
    if (!a.count_atomics || ABL(16384)) return;
    const float nf = (float)__builtin_amdgcn_readfirstlane(n_flush), nd = wave_sum((float)n_direct);
    float *cnt = a.loss_acc + 8 + 2 * (r & 63);
    if (lane == 0 && nf != 0.f) atomic_add_f32(cnt, nf);
    if (lane == 0 && nd != 0.f) atomic_add_f32(cnt + 1, nd);
}

// xy-quad mirror of the fp16 table for k_encode (amp, dense levels): quad r = the fp16 pairs of
// rows {r, r+1, r+rs, r+rs+1} of r's level (rs = res + 1), i.e. the corners (x, y), (x+1, y),
// (x, y+1), (x+1, y+1) of the cell whose (x, y, z) corner is row r. A cell's 8 corners are then
// the quads at its base row and base + rs^2: two 16-B loads instead of four 8-B pair loads
// (k_encode's corner gathers are bound by L1 line accesses: 26 per sample with pairs). Rebuilt
// from the mirror at the start of every field pass (the optimiser / all-gather update the
// pairs); rows whose quad would leave the level (never a cell corner) and hashed levels are
// not written. One row per thread (16-B stores of consecutive lanes are contiguous; four rows per
// thread with one 16-B load each measured 49 vs 29 us at the headline).
__global__ __launch_bounds__(256) void k_quad_mirror(FieldArgs a) {
    // persistent grid over the dense levels' rows (a prefix of the table: levels are stored
    // coarse to fine and a level is dense up to its first hashed one); the level records in LDS,
    // each thread's level advanced as its rows grow (a per-block scalar walk from level 0 was a
    // dependent load chain per 256 rows)
    __shared__ uint32_t s_off[16], s_rs[16], s_end[16];
    if (threadIdx.x < a.L) {
        const LevelInfo li = level_info(a, threadIdx.x);
        s_off[threadIdx.x] = li.off;
        s_rs[threadIdx.x] = li.res + 1;
        s_end[threadIdx.x] = level_dense(li.res + 1, li.hs) ? li.off + li.hs : 0u;
    }
    __syncthreads();
    uint32_t end = 0;
    for (int l = 0; l < (int)a.L && s_end[l]; ++l) end = s_end[l];
    const uint32_t *t = reinterpret_cast<const uint32_t *>(a.table);
    uint4 *quads = const_cast<uint4 *>(a.quads);
    int lv = 0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < end; i += gridDim.x * 256u) {
        while (lv + 1 < (int)a.L && s_off[lv + 1] <= i) ++lv;
        const uint32_t rs = s_rs[lv], hi = i + rs + 1;
        if (hi >= s_end[lv]) continue;   // the quad would leave the level: never a cell corner
        quads[i] = make_uint4(t[i], t[i + 1], t[i + rs], t[hi]);
    }
}

__global__ void k_zero_i32(int *__restrict__ p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}

// ---------------------------------------------------- ray setup + trace
__global__ __launch_bounds__(256) void k_trace(const float *__restrict__ pool, const int32_t *__restrict__ ids, int R,
                                               const float *__restrict__ tf, const uint8_t *__restrict__ occ, int N,
                                               int Kmax, float near_sc, float far_sc, float trunc,
                                               float *__restrict__ rays_out, float *__restrict__ intervals,
                                               float *__restrict__ totals, int32_t *__restrict__ counts,
                                               const nof_step_params *__restrict__ sp,
                                               const int32_t *__restrict__ epoch_step0) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    if (sp) trunc = sp->trunc;
    // epoch permutation (nof_trace_rays_epoch): this step's slice, from the device step block
    if (epoch_step0) ids += (size_t)(sp->step - *epoch_step0) * (size_t)R;
    const float *src = pool + (size_t)(ids ? ids[r] : r) * 12;
    float ray[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) ray[k] = src[k];
    if (ids) {
#pragma unroll
        for (int k = 0; k < 12; ++k) rays_out[(size_t)r * 12 + k] = ray[k];
    }
    const float nrm = sqrtf((ray[0] * ray[0] + ray[1] * ray[1]) + ray[2] * ray[2]);
    const float vd[3] = {ray[0] / nrm, ray[1] / nrm, ray[2] / nrm};
    const float *T = tf + (size_t)((int)ray[8]) * 16;
    const float o[3] = {T[3], T[7], T[11]};
    float d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = (T[i * 4] * vd[0] + T[i * 4 + 1] * vd[1]) + T[i * 4 + 2] * vd[2];
    float *dst = intervals + (size_t)r * Kmax * 2;
    // depths_in_out -> z (sample_rays_uniform_occupied_voxels :986-998; note the second normalisation),
    // applied to each interval as the trace emits it (no read-back of the written intervals)
    const float n2 = sqrtf((vd[0] * vd[0] + vd[1] * vd[1]) + vd[2] * vd[2]);
    const float vz = fabsf(vd[2] / n2);
    const float depth = ray[6];
    const bool vdepth = (depth >= near_sc) && (depth <= far_sc);
    const float hi = depth + trunc;
    float total = 0.f;
    const int k = trace_ray_emit(occ, N, o, d, Kmax, [&](int j, float tin, float tout) {
        float zi = tin * vz, zo = tout * vz;
        if (vdepth && zi > 0.f && zo > 0.f) {
            zi = fminf(fmaxf(zi, 0.f), hi);
            zo = fminf(fmaxf(zo, 0.f), hi);
        }
        *reinterpret_cast<float2 *>(dst + j * 2) = make_float2(zi, zo);
        total += zo - zi;
    });
    // one zero entry ends the list (sample_z's walk stops at the first zero z_in, as the reference's
    // common.cu walk over its zero-padded depths_in_out): the rest of the row is never read, and
    // zero-padding all Kmax entries was most of this kernel's HBM writes
    if (k < Kmax) *reinterpret_cast<float2 *>(dst + k * 2) = make_float2(0.f, 0.f);
    totals[r] = total;
    if (counts) counts[r] = k;
}

// ------------------------------------------------------------ MLP pack
template <typename TM>
__global__ __launch_bounds__(256) void k_pack_mlp(const float *__restrict__ mlp, const int32_t *__restrict__ idx,
                                                  int n_frag_elems, int n_bias, TM *__restrict__ frags,
                                                  float *__restrict__ bias) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_frag_elems) {
        const int k = idx[i];
        frags[i] = (TM)(k >= 0 ? mlp[k] : 0.f);
    } else if (i < n_frag_elems + n_bias) {
        const int k = idx[i];
        bias[i - n_frag_elems] = k >= 0 ? mlp[k] : 0.f;
    }
}

// -------------------------------------------------------------- batch
// Throughput-mode ray selection: rays_per_frame uniform draws (with replacement)
// inside each frame's contiguous pool segment (frame_start [F+1]), one block per frame,
// produced already in ascending pool (raster) order, so neighbouring waves trace neighbouring
// pixels and share their table rows in L2. The k sorted draws are generated directly as the
// order statistics of k uniforms: U_(j) = S_j / S_k with S_j = E_0 + ... + E_j the prefix sums
// of k + 1 exponential variates (E = -log u, counter-hash u) — one block-wide prefix sum
// instead of a bitonic sort of the draws (66 barrier stages for 2048: ~26 us per step on the
// 64 frames' blocks); id_j = lo + floor(cnt U_(j)) has the distribution of k sorted iid
// uniform draws from the frame's rays.
constexpr int SAMPLE_BATCH_MAX = 4096;
__global__ __launch_bounds__(1024) void k_sample_batch(const int64_t *__restrict__ frame_start, int F,
                                                      int rays_per_frame, uint32_t seed, int32_t *__restrict__ ids,
                                                      const nof_step_params *__restrict__ sp) {
    if (sp) seed = sp->batch_seed;
    __shared__ float s_t[1024];
    const int f = blockIdx.x, t = threadIdx.x;
    const int k = rays_per_frame, m = k + 1;
    const int chunk = (m + 1023) / 1024;   // <= 5 (rays_per_frame <= 4096)
    const int j0 = t * chunk, j1 = min(m, j0 + chunk);
    const int64_t lo = frame_start[f], cnt = frame_start[f + 1] - lo;
    // this thread's exponential variates, their running sum
    float e[5];
    float run = 0.f;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        e[q] = 0.f;
        const int j = j0 + q;
        if (q < chunk && j < j1) {
            const uint32_t i = (uint32_t)(f * m + j);
            const uint32_t u = hash32(seed ^ hash32(i * 0x85EBCA6BU + 0x27D4EB2FU));
            e[q] = -__logf(((float)u + 0.5f) * 2.3283064e-10f);   // u in (0, 1)
            run += e[q];
        }
    }
    // block-wide inclusive scan of the threads' sums (Hillis-Steele in LDS)
    s_t[t] = run;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const float x = s_t[t] + (t >= off ? s_t[t - off] : 0.f);
        __syncthreads();
        s_t[t] = x;
        __syncthreads();
    }
    const float total = s_t[1023];
    float acc = t > 0 ? s_t[t - 1] : 0.f;
    const float scale = (float)cnt / total;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const int j = j0 + q;
        if (q < chunk && j < min(j1, k)) {   // S_j for j < k (S_k = total, the normaliser)
            acc += e[q];
            int64_t id = (int64_t)(acc * scale);
            id = (id < 0 || cnt <= 0) ? 0 : (id >= cnt ? cnt - 1 : id);
            ids[(size_t)f * k + j] = (int32_t)(lo + id);
        }
    }
}

}  // namespace nof

extern "C" int nof_trace_rays(const float *pool, const int32_t *ids, int32_t R, const float *tf, const uint8_t *occ,
                              int32_t N, int32_t Kmax, float near_sc, float far_sc, float trunc, float *rays_out,
                              float *intervals, float *totals, int32_t *counts, const nof_step_params *sp,
                              void *stream) {
    if (R <= 0) return NOF_OK;
    if (N <= 0 || Kmax <= 0) return nof::set_error(NOF_EINVAL, "trace_rays: bad N=%d Kmax=%d", N, Kmax);
    // one lane per ray: small batches (NerfRunner.train's 2048 rays) in 64-lane blocks, so the rays'
    // serial DDA chains spread over 32 CUs instead of 8
    const int tb = R >= 65536 ? 256 : 64;
    hipLaunchKernelGGL(nof::k_trace, dim3(nof::div_up(R, tb)), dim3(tb), 0, (hipStream_t)stream, pool, ids, R, tf,
                       occ, N, Kmax, near_sc, far_sc, trunc, rays_out, intervals, totals, counts, sp,
                       (const int32_t *)nullptr);
    return nof::check_launch("trace_rays");
}

extern "C" int nof_trace_rays_epoch(const float *pool, const int32_t *perm, const int32_t *epoch_step0, int32_t R,
                                    const float *tf, const uint8_t *occ, int32_t N, int32_t Kmax, float near_sc,
                                    float far_sc, float trunc, float *rays_out, float *intervals, float *totals,
                                    int32_t *counts, const nof_step_params *sp, void *stream) {
    if (R <= 0) return NOF_OK;
    if (!perm || !epoch_step0 || !sp)
        return nof::set_error(NOF_EINVAL, "trace_rays_epoch: perm, epoch_step0 and the step block are required");
    if (N <= 0 || Kmax <= 0) return nof::set_error(NOF_EINVAL, "trace_rays_epoch: bad N=%d Kmax=%d", N, Kmax);
    const int tb = R >= 65536 ? 256 : 64;
    hipLaunchKernelGGL(nof::k_trace, dim3(nof::div_up(R, tb)), dim3(tb), 0, (hipStream_t)stream, pool, perm, R, tf,
                       occ, N, Kmax, near_sc, far_sc, trunc, rays_out, intervals, totals, counts, sp, epoch_step0);
    return nof::check_launch("trace_rays_epoch");
}

extern "C" int nof_pack_mlp(const float *mlp, const int32_t *idx, int32_t n_frag_elems, int32_t n_bias, void *frags,
                            float *bias, int mlp_dtype, void *stream) {
    const int n = n_frag_elems + n_bias;
    if (mlp_dtype == NOF_F16)
        hipLaunchKernelGGL(nof::k_pack_mlp<_Float16>, dim3(nof::div_up(n, 256)), dim3(256), 0, (hipStream_t)stream,
                           mlp, idx, n_frag_elems, n_bias, (_Float16 *)frags, bias);
    else
        hipLaunchKernelGGL(nof::k_pack_mlp<float>, dim3(nof::div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, mlp,
                           idx, n_frag_elems, n_bias, (float *)frags, bias);
    return nof::check_launch("pack_mlp");
}

extern "C" int nof_sample_batch(const int64_t *frame_start, int32_t F, int32_t rays_per_frame, uint32_t seed,
                                int32_t *ids, const nof_step_params *sp, void *stream) {
    const int n = F * rays_per_frame;
    if (n <= 0) return NOF_OK;
    if (rays_per_frame > nof::SAMPLE_BATCH_MAX)
        return nof::set_error(NOF_EINVAL, "sample_batch: rays_per_frame %d > %d", rays_per_frame,
                              nof::SAMPLE_BATCH_MAX);
    // one block of 1024 threads per frame: the bitonic stages run 2 compare-swaps per thread
    // (256 threads took 8 per stage, ~60 us per 64-frame batch)
    hipLaunchKernelGGL(nof::k_sample_batch, dim3(F), dim3(1024), 0, (hipStream_t)stream, frame_start,
                       F, rays_per_frame, seed, ids, sp);
    return nof::check_launch("sample_batch");
}

namespace {
// Optional per-kernel timing (nof_field_timing): one set of events per call,
// recorded on the launch stream between the kernels.
constexpr int N_FIELD_KERNELS = 4;   // encode, mlp_fwd (+ compact), mlp_bwd (2 passes), scatter
struct FieldTiming {
    bool on = false;
    std::vector<std::array<hipEvent_t, N_FIELD_KERNELS + 1>> sets;
    size_t used = 0;
};
FieldTiming g_timing;
hipEvent_t *timing_set() {
    if (!g_timing.on) return nullptr;
    if (g_timing.used == g_timing.sets.size()) {
        std::array<hipEvent_t, N_FIELD_KERNELS + 1> e{};
        for (auto &x : e)
            if (hipEventCreate(&x) != hipSuccess) return nullptr;
        g_timing.sets.push_back(e);
    }
    return g_timing.sets[g_timing.used++].data();
}
inline void mark(hipEvent_t *ev, int i, hipStream_t st) {
    if (ev) (void)hipEventRecord(ev[i], st);
}

template <typename TM, typename TT, bool DBG>
auto encode_kernel(int g) {
    return g == 4 ? nof::k_encode<TM, TT, 4, DBG> : (g == 2 ? nof::k_encode<TM, TT, 2, DBG> : nof::k_encode<TM, TT, 1, DBG>);
}

template <typename TM, typename TT, int WPB>
int launch_field(const nof::FieldArgs &a, int n_cu, hipStream_t st) {
    const int ntiles = a.S / 32;
    // the record counter and the loss rows (contiguous in the workspace) are reset by a kernel, not
    // a memset: the step is captured into a hipGraph, and kernel nodes are the only node kind it holds
    hipLaunchKernelGGL(nof::k_ray_ctx, dim3(nof::div_up(a.R, 256)), dim3(256), 0, st, a);
    hipEvent_t *ev = timing_set();
    mark(ev, 0, st);
    if (a.quads && !a.quads_ready)   // amp, large batches: the encode's xy-quad mirror (timed with k_encode)
        hipLaunchKernelGGL(nof::k_quad_mirror, dim3(nof::tile_blocks(a.n_rows, 256, n_cu, 8)), dim3(256), 0, st, a);
    // encode + sigma net: 8-wave blocks (the layer-1 / 2 fragments staged once per 8 tiles)
    // weights + biases + 8 waves' level tables (16 levels x 32 B)
    const size_t elds = (size_t)8 * 64 * 8 * sizeof(TM) + 2 * 64 * sizeof(float) + 8 * 16 * 32;
    {
        const dim3 eg(nof::div_up((uint64_t)a.R * ntiles, 8));
        const bool dbg = a.dbg_z || a.dbg_valid || a.dbg_raw;
        hipLaunchKernelGGL((dbg ? encode_kernel<TM, TT, true>(a.encode_group) : encode_kernel<TM, TT, false>(a.encode_group)),
                           eg, dim3(512), elds, st, a);
    }
    int rc = nof::check_launch("field_step(encode)");
    if (rc) return rc;
    mark(ev, 1, st);
    // tile-parallel colour forward: the colour-tile list comes from the same compaction pass as
    // the backward list (the flags are final after k_encode)
    {
        const int nflags = a.R * ntiles;
        const int per = a.compact_per > 0 ? a.compact_per : (nflags >= 262144 ? nof::COMPACT_PER_BLOCK : 512);
        hipLaunchKernelGGL(nof::k_compact, dim3(nof::div_up((uint64_t)nflags, per)), dim3(256), 0, st, a.tile_bwd,
                           nflags, a.tile_sid, a.n_tiles, per, a.ctile_list);
        rc = nof::check_launch("field_step(compact)");
        if (rc) return rc;
        // 4-wave blocks, 6 per CU (6 waves per SIMD at 80 registers; 17 KB of colour-net fragments per block):
        // 5 per CU measured 0.249 / 0.247 ms, 6 0.237 / 0.234, 8 (64 registers, spilling) 0.394 (profiles/r5/ab_r5m_*)
        constexpr int WPB_C = 4;
        const int nbc = std::max(1, nof::tile_blocks(nflags, 8, n_cu, 6));
        const size_t clds = nof::staged_bytes<TM, nof::COL_NFR>();
        hipLaunchKernelGGL((a.dbg_raw ? nof::k_colour<TM, WPB_C, 6, true> : nof::k_colour<TM, WPB_C, 6, false>), dim3(nbc),
                           dim3(WPB_C * 64), clds, st, a);
        rc = nof::check_launch("field_step(colour)");
        if (rc) return rc;
        hipLaunchKernelGGL(nof::k_ray_final, dim3(nof::div_up(a.R, 256)), dim3(256), 0, st, a);
        rc = nof::check_launch("field_step(ray_final)");
        if (rc) return rc;
    }
    mark(ev, 2, st);
    // + 16 floats: k_mlp_bwd's per-wave frame-feature gradient sums
    const size_t mlds = nof::staged_bytes<TM, nof::N_FRAGS>(false, 16 * sizeof(float));
    if constexpr (sizeof(TM) == 2) {
        // amp: the weight gradients take their K = samples operands from LDS transposes
        // (k_mlp_bwd_tr): 8-wave blocks (12 KB of images per wave), one per CU
        // the weight gradients summed over the 8-wave block before the atomics (8 x fewer; bwd_flush 0 / 2,
        // the default; 1: one atomic per element per wave), the grid widened to every CU. Measured
        // against the per-wave flush (round 4, same box): 2048 rays 0.351 ->
        // 0.306 ms per step, 16 K rays 0.255 -> 0.161 ms, 32 K 0.372 -> 0.309, 64 K 0.603 -> 0.576,
        // the 131 K-ray headline 1.109 -> 1.086 and 1.123 -> 1.107 ms
        const int64_t nt_all = (int64_t)a.R * ntiles;
        const bool blk = a.bwd_flush != 1;
        const int nbt = std::max(1, nof::tile_blocks(nt_all, blk ? 48 : 128, n_cu, 1));
        const size_t tl0 = nof::bwd_tr_lds(0, 8), tl1 = nof::bwd_tr_lds(1, 8);
        const auto tr0 = a.n_ff > 0 ? (blk ? nof::k_mlp_bwd_tr<8, 0, true, true> : nof::k_mlp_bwd_tr<8, 0, true>)
                                    : (blk ? nof::k_mlp_bwd_tr<8, 0, false, true> : nof::k_mlp_bwd_tr<8, 0>);
        hipLaunchKernelGGL(tr0, dim3(nbt), dim3(8 * 64), tl0, st, a);
        rc = nof::check_launch("field_step(mlp_bwd_tr0)");
        if (rc) return rc;
        hipLaunchKernelGGL((blk ? nof::k_mlp_bwd_tr<8, 1, false, true> : nof::k_mlp_bwd_tr<8, 1>), dim3(nbt), dim3(8 * 64), tl1, st, a);
        rc = nof::check_launch("field_step(mlp_bwd_tr1)");
        if (rc) return rc;
    } else {
        // fp32 (parity mode): two persistent passes of 4-wave blocks; small batches get fewer persistent
        // waves (~16 tiles of the batch per wave), so the per-wave weight-gradient atomics at the end do
        // not outweigh the tiles. Pass 1 would spill at 2 waves per SIMD in fp32 and keeps one.
        const int nbb = std::max(1, nof::tile_blocks((int64_t)a.R * ntiles, 64, n_cu, 2));
        hipLaunchKernelGGL((nof::k_mlp_bwd<TM, 4, 2, 0>), dim3(nbb), dim3(4 * 64), mlds, st, a);
        rc = nof::check_launch("field_step(mlp_bwd0)");
        if (rc) return rc;
        const int nb1 = std::min(nbb, n_cu);
        hipLaunchKernelGGL((a.n_ff > 0 ? nof::k_mlp_bwd<TM, 4, 1, 1, true> : nof::k_mlp_bwd<TM, 4, 1, 1>), dim3(nb1), dim3(4 * 64), mlds, st, a);
        rc = nof::check_launch("field_step(mlp_bwd)");
        if (rc) return rc;
    }
    mark(ev, 3, st);
    const int n_grp = ((int)a.L + a.scatter_lpw - 1) / a.scatter_lpw;
    const dim3 sg(nof::div_up((uint64_t)a.R * n_grp, 4));
    // per-ray table accumulation in LDS: amp adds packed fp16x2 (the reference's __half2
    // atomicAdd per sample and corner, gridencoder.cu:319-327, rounds once per sample; here
    // once per DPP run of samples — 0.16 ms less per config-2 step than fp32 pairs), fp32
    // mode adds fp32 pairs
    if constexpr (sizeof(TM) == 2) {
        const size_t lds = (size_t)4 * 4 * nof::scatter_wave_words(a.slot_mask, 1);
        hipLaunchKernelGGL((nof::k_scatter<TM, TT, true, 7>), sg, dim3(256), lds, st, a);
    } else {
        hipLaunchKernelGGL((nof::k_scatter<TM, TT, false, 1>), sg, dim3(256),
                           (size_t)4 * 4 * nof::scatter_wave_words(a.slot_mask, 2), st, a);
    }
    rc = nof::check_launch("field_step(scatter)");
    if (rc) return rc;
    mark(ev, 4, st);
    return NOF_OK;
}

// The step's workspace: the size export reads `bytes`, nof_field_workspace_offsets `off`, the step the pointers.
// part<I, T> is section I of NOF_WS_SECTIONS (include/nof.h names them in this order); the last is the total.
struct FieldWorkspace : nof::Carver {
    void *feat, *dfeat;
    float *zbuf, *ray_aux, *rctx, *rrec;
    uint8_t *tile_bwd;
    int *tile_sid, *n_tiles, *ctile;
    float4 *tile_aux;
    uint32_t *gmask;
    uint64_t off[NOF_WS_SECTIONS] = {};
    template <int I, typename T> T *part(size_t count) {
        static_assert(I < NOF_WS_SECTIONS - 1, "a new section needs a larger NOF_WS_SECTIONS in include/nof.h");
        return off[I] = bytes, take<T>(count);
    }
    FieldWorkspace(void *base, int R, int S, int mlp_dtype) : Carver(base) {
        const size_t el = mlp_dtype == NOF_F16 ? 2 : 4, n = (size_t)R * S, nt = (size_t)R * (S / 32);
        feat = part<0, char>(n * 32 * el);
        dfeat = part<1, char>(n * 32 * el);
        zbuf = part<2, float>(n);
        tile_bwd = part<3, uint8_t>(nt);
        tile_sid = part<4, int>(nt);
        n_tiles = part<5, int>(nof::LOSS_ZERO_WORDS);   // + the loss rows (folded by the scatter kernel)
        ray_aux = part<6, float>((size_t)R * nof::RAY_AUX);
        tile_aux = part<7, float4>(nt * nof::TILE_AUX);
        rctx = part<8, float>((size_t)R * nof::RCTX);
        gmask = part<9, uint32_t>(nt);
        rrec = part<10, float>(nt * nof::TREC);
        ctile = part<11, int>(nt);
        off[NOF_WS_SECTIONS - 1] = bytes;
    }
};
// the encode's xy-quad mirror: amp, batches large enough to repay its per-step rebuild (~25 us)
bool quads_on(const nof_field_desc *d) {
    return d->table_quads && d->table_rows > 0 && d->mlp_dtype == NOF_F16 && d->table_dtype == NOF_F16 &&
           d->R >= (d->quads_min_rays > 0 ? d->quads_min_rays : 32768) && !ABL_HOST(d, 512);
}
}  // namespace

extern "C" size_t nof_field_workspace_bytes(int32_t R, int32_t S, int32_t mlp_dtype) {
    return FieldWorkspace(nullptr, R, S, mlp_dtype).bytes;
}

extern "C" int nof_field_workspace_offsets(int32_t R, int32_t S, int32_t mlp_dtype, uint64_t *offsets, int32_t n) {
    if (R < 0 || S <= 0 || !offsets || n < NOF_WS_SECTIONS)
        return nof::set_error(NOF_EINVAL, "field_workspace_offsets: bad R=%d S=%d or n=%d < %d", R, S, n,
                              NOF_WS_SECTIONS);
    const FieldWorkspace w(nullptr, R, S, mlp_dtype);
    for (int i = 0; i < NOF_WS_SECTIONS; ++i) offsets[i] = w.off[i];
    return NOF_OK;
}

extern "C" size_t nof_field_desc_size(void) { return sizeof(nof_field_desc); }

extern "C" int nof_quad_mirror(const nof_field_desc *d, void *stream) {
    if (!d) return nof::set_error(NOF_EINVAL, "quad_mirror: desc is NULL");
    if (d->L > 16 || d->C != 2)
        return nof::set_error(NOF_EINVAL, "quad_mirror: needs C=2, L<=16 (got %u,%u)", d->C, d->L);
    if (d->R <= 0 || !quads_on(d)) return NOF_OK;   // the step would not read the mirror
    nof::FieldArgs a{};
    a.table = d->table; a.levels = (const float4 *)d->levels; a.L = d->L;
    a.quads = (const uint4 *)d->table_quads; a.n_rows = (uint32_t)d->table_rows;
    hipLaunchKernelGGL(nof::k_quad_mirror, dim3(nof::tile_blocks(a.n_rows, 256, nof::cu_count(), 8)), dim3(256), 0,
                       (hipStream_t)stream, a);
    return nof::check_launch("quad_mirror");
}

extern "C" int nof_field_step(const nof_field_desc *d, void *stream) {
    if (!d) return nof::set_error(NOF_EINVAL, "field_step: desc is NULL");
    if (d->S % 32 != 0 || d->S > 320 || d->N_oct + d->N_dep != d->S)
        return nof::set_error(NOF_EINVAL, "field_step: S=%d must be N_oct+N_dep, a multiple of 32, <= 320", d->S);
    if (int rc = nof::check_geometry("field_step", d, false)) return rc;
    if (d->R <= 0) return NOF_OK;
    // every refusal comes before the first HIP call: a bad descriptor costs no device work
    if (d->bwd_flush < 0 || d->bwd_flush > 2)
        return nof::set_error(NOF_EINVAL, "field_step: bwd_flush %d (0 by batch size, 1 per wave, 2 block)", d->bwd_flush);
    if (d->compact_per_block != 0 && (d->compact_per_block < 256 || d->compact_per_block > nof::COMPACT_PER_BLOCK ||
                                      d->compact_per_block % 256 != 0))
        return nof::set_error(NOF_EINVAL, "field_step: compact_per_block %d (0 by batch size, else a multiple of 256 "
                              "in [256, %d])", d->compact_per_block, nof::COMPACT_PER_BLOCK);
    if (d->encode_group != 0 && d->encode_group != 1 && d->encode_group != 2 && d->encode_group != 4)
        return nof::set_error(NOF_EINVAL, "field_step: encode_group %d (0 by batch size, or 1, 2, 4)", d->encode_group);
    if (int rc = nof::check_frame_features("field_step", d->n_ff, d->ff, d->grad_ff, true)) return rc;
    if (d->mlp_dtype == NOF_F16 && !d->grad_table16)
        return nof::set_error(NOF_EINVAL, "field_step: amp mode needs grad_table16 (fp16 table gradient)");
    if (d->ablate && !NOF_ABLATE)
        return nof::set_error(NOF_EINVAL, "field_step: ablate bits need a -DNOF_ABLATE=1 build (timing experiments only)");
    if (!d->workspace) return nof::set_error(NOF_EINVAL, "field_step: workspace is NULL (nof_field_workspace_bytes)");
    const int slots = d->scatter_slots ? d->scatter_slots : 512;
    if (slots < 64 || slots > 2048 || (slots & (slots - 1)))
        return nof::set_error(NOF_EINVAL, "field_step: scatter_slots must be a power of two in [64, 2048]");
    bool amp;
    if (int rc = nof::check_dtype_pair("field_step", d, amp)) return rc;

    nof::FieldArgs a;
    nof::fill_sampling(a, d);
    nof::fill_model(a, d);
    a.t_rand = d->t_rand; a.seed = d->seed; a.perturb = d->perturb;
    a.fs_sdf = d->fs_sdf; a.ffw = d->first_frame_weight;
    a.rgb_w = d->rgb_weight; a.fs_w = d->fs_weight; a.empty_w = d->empty_weight; a.trunc_w = d->trunc_weight;
    a.inv_3R = 1.0f / (3.0f * (float)d->R);
    a.inv_RS = 1.0f / ((float)d->R * (float)d->S);
    a.inv_3RS = 1.0f / (3.0f * (float)d->R * (float)d->S);
    a.xcd_order = d->xcd_order;
    a.no_dx = d->skip_pose_grad != 0;
    a.quads = quads_on(d) ? (const uint4 *)d->table_quads : nullptr;
    a.n_rows = (uint32_t)d->table_rows;
    a.quads_ready = d->quads_prebuilt != 0;
    {   // k_scatter: a wave per (ray, level group). Measured optimum (scripts/ablate.py LPW sweep,
        // DESIGN §4): a wave per ray from 192 K rays (config 5's 258 K: 13.2 vs 13.7 ms with 8),
        // 8 levels per wave from 32 K (the headline: 2.36 -> 2.29 ms vs a wave per ray; at 8 waves per
        // SIMD, round 6: 1.879 vs 1.917 ms, and config 2's 32 K rays 0.495 vs 0.512 ms with 4), 4 from
        // 8 K (16 K rays: 0.37 -> 0.33 ms vs 8; round 6: 0.294 vs 0.306), 2 below (NerfRunner.train's
        // 2048 rays: 0.418 -> 0.395 ms per step vs 1)
        const int L = std::max(1, (int)d->L);
        const int want = d->R >= 196608 ? 16 : (d->R >= 32768 ? 8 : (d->R >= 8192 ? 4 : 2));
        a.scatter_lpw = std::max(1, std::min(L, d->scatter_levels_per_wave > 0 ? (int)d->scatter_levels_per_wave : want));
    }
    a.bwd_flush = d->bwd_flush;
    a.count_atomics = d->count_atomics != 0;
    a.compact_per = d->compact_per_block;
    a.encode_group = d->encode_group ? d->encode_group : (d->R >= 8192 ? 1 : nof::ENCODE_GROUP_SMALL);
    a.sp = d->step_params;
    a.fs_rgb_w = d->fs_rgb_weight;
    a.loss_scale = d->loss_scale; a.grad_ff = d->grad_ff;
    a.grad_table = d->grad_table; a.grad_mlp = d->grad_mlp;
    a.grad_table16 = (__half *)d->grad_table16;
    a.ray_grad = d->ray_grad; a.loss_acc = d->loss_acc; a.dbg_z = d->dbg_z; a.dbg_raw = d->dbg_raw;
    a.dbg_valid = d->dbg_valid; a.dbg_rgb = d->dbg_rgb; a.ablate = d->ablate;
    a.slot_mask = (uint32_t)slots - 1;
    const FieldWorkspace ws(d->workspace, d->R, d->S, d->mlp_dtype);
    a.feat = ws.feat; a.dfeat = ws.dfeat; a.zbuf = ws.zbuf; a.tile_bwd = ws.tile_bwd; a.tile_sid = ws.tile_sid;
    a.n_tiles = ws.n_tiles; a.loss_part = (float *)ws.n_tiles + 16;   // the loss rows follow the counters in their part
    a.ray_aux = ws.ray_aux; a.tile_aux = ws.tile_aux; a.rctx = ws.rctx; a.tile_gmask = ws.gmask; a.rrec = ws.rrec;
    a.ctile_list = ws.ctile;

    hipStream_t st = (hipStream_t)stream;
    const int n_cu = nof::cu_count();
    return amp ? launch_field<_Float16, __half, 4>(a, n_cu, st) : launch_field<float, float, 4>(a, n_cu, st);
}

extern "C" int nof_field_timing(int32_t enable) {
    g_timing.on = enable != 0;
    g_timing.used = 0;
    return NOF_OK;
}

extern "C" int nof_field_timing_collect(float *ms_sum, int32_t n, int32_t *calls) {
    if (!ms_sum || n < N_FIELD_KERNELS) return nof::set_error(NOF_EINVAL, "field_timing_collect: need 4 floats");
    for (int k = 0; k < n; ++k) ms_sum[k] = 0.f;
    for (size_t i = 0; i < g_timing.used; ++i) {
        auto &e = g_timing.sets[i];
        if (hipEventSynchronize(e[N_FIELD_KERNELS]) != hipSuccess)
            return nof::set_error(NOF_ELAUNCH, "field_timing_collect: event sync failed");
        for (int k = 0; k < N_FIELD_KERNELS; ++k) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e[k], e[k + 1]) != hipSuccess)
                return nof::set_error(NOF_ELAUNCH, "field_timing_collect: elapsed time failed");
            ms_sum[k] += ms;
        }
    }
    if (calls) *calls = (int32_t)g_timing.used;
    g_timing.used = 0;
    return NOF_OK;
}
