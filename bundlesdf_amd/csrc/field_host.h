// Host helpers of the field entry points, shared by field_step.hip and field_infer.hip. Host only;
// include nothing after field_core.h that minds floating-point contraction (its pragma stays in force).
#pragma once
#include <algorithm>

#include "field_core.h"
#include "host_entry.h"

namespace nof {

// compute units of the current device (the persistent grids' size); 256, the MI355X's, when the query fails
inline int cu_count() {
    int dev = 0, n_cu = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        n_cu = 256;
    return n_cu;
}
// blocks of a grid that takes per_block of n work items a block, persistent from per_cu blocks per CU
inline int tile_blocks(int64_t n, int per_block, int n_cu, int per_cu) {
    return (int)std::min<int64_t>((n + per_block - 1) / per_block, (int64_t)n_cu * per_cu);
}

// f(tag) with the kernels' template types (TM the MLP's element type, TT the table's), and one launch of
// the kernel template K<TM, TT> through it; `lds` may name TM
template <typename M, typename T> struct DtypeTag { typedef M TM; typedef T TT; };
template <typename F> inline void dispatch_dtype(bool amp, F &&f) {
    if (amp) f(DtypeTag<_Float16, __half>{});
    else f(DtypeTag<float, float>{});
}
#define NOF_LAUNCH_TYPED(amp, K, grid, block, lds, st, ...) \
    nof::dispatch_dtype(amp, [&](auto tag_) {                                 \
        typedef typename decltype(tag_)::TM TM; typedef typename decltype(tag_)::TT TT; \
        hipLaunchKernelGGL((K<TM, TT>), grid, block, (lds), st, __VA_ARGS__); \
    })

// The field model's descriptor checks, one per refusal (the entry points run them in different orders, and
// the first refusal is what a caller sees). `who` prefixes the message; NOF_OK or set_error's code; no HIP call.
inline int check_geometry(const char *who, const nof_field_desc *d, bool need_level) {   // need_level: L == 0 refused
    if (!(need_level && d->L == 0) && d->L <= 16 && d->C == 2 && d->D == 3) return NOF_OK;
    return set_error(NOF_EINVAL, "%s: needs D=3, C=2, %sL<=16 (got %u,%u,%u)", who, need_level ? "1<=" : "", d->D, d->C, d->L);
}
inline int check_dtype_pair(const char *who, const nof_field_desc *d, bool &amp) {
    amp = d->mlp_dtype == NOF_F16 && d->table_dtype == NOF_F16;
    return amp || (d->mlp_dtype == NOF_F32 && d->table_dtype == NOF_F32)
               ? NOF_OK : set_error(NOF_EINVAL, "%s: mlp/table dtype must both be f16 (amp) or both f32", who);
}
inline int check_model_pointers(const char *who, const nof_field_desc *d) {
    return d->table && d->levels && d->frags && d->bias
               ? NOF_OK : set_error(NOF_EINVAL, "%s: table / levels / frags / bias is NULL", who);
}
inline int check_frame_features(const char *who, int n_ff, const float *ff, const float *grad_ff = nullptr,
                                bool grad_too = false) {   // grad_too: the step needs the gradient array as well
    if (n_ff >= 0 && n_ff <= 3 && (n_ff == 0 || (ff && (!grad_too || grad_ff)))) return NOF_OK;
    return set_error(NOF_EINVAL, "%s: frame_features must be 0..3 with ff%s set (got %d)", who, grad_too ? " and grad_ff" : "", n_ff);
}

// the field-model part of FieldArgs, from the loose arguments of the query calls or a descriptor
inline void fill_model(FieldArgs &a, const void *table, const float *levels, uint32_t L, int mlp_in, const void *frags,
                       const float *bias, int n_ff = 0, const float *ff = nullptr) {
    a.table = table; a.levels = reinterpret_cast<const float4 *>(levels); a.L = L; a.mlp_in = mlp_in;
    a.frags = frags; a.bias = bias; a.n_ff = n_ff; a.ff = ff;
}
inline void fill_model(FieldArgs &a, const nof_field_desc *d) {
    fill_model(a, d->table, d->levels, d->L, (int)(d->L * d->C), d->frags, d->bias, d->n_ff, d->ff);
}
// the sampling block the step and the ray render share
inline void fill_sampling(FieldArgs &a, const nof_field_desc *d) {
    a.rays = d->rays; a.tf = d->tf; a.intervals = d->intervals; a.totals = d->totals;
    a.R = d->R; a.Kmax = d->Kmax; a.N_oct = d->N_oct; a.N_dep = d->N_dep; a.S = d->S; a.trunc = d->trunc;
    a.near_sc = d->near_sc; a.far_sc = d->far_sc; a.ntr = d->neg_trunc_ratio; a.lambda = d->sdf_lambda;
}

}  // namespace nof
