// The inference side of the field model for gfx950 (CDNA4): the host entry points and workspaces of the
// SDF and point queries (field_query.h), the forward-only ray render (field_render.h) and the free-camera
// surface render (field_view.h), whose kernels sit on the device core they share with the training step
// (field_core.h). No kernel here uses an atomic: two calls on the same inputs are bit-identical.
#include "field_core.h"
#include "field_host.h"
#include "field_query.h"
#include "field_render.h"
#include "field_view.h"

#pragma clang fp contract(off)

namespace {
int query_blocks(int64_t n) { return nof::tile_blocks((n + 31) / 32, 4, nof::cu_count(), 2); }
void launch_query_sdf(bool amp, const nof::FieldArgs &a, const nof::QueryArgs &q, hipStream_t st) {
    NOF_LAUNCH_TYPED(amp, nof::k_query_sdf, dim3(query_blocks(q.n)), dim3(256), (nof::staged_bytes<TM, nof::N_FRAGS>()), st, a, q);
}
}  // namespace

extern "C" int nof_query_sdf(const void *table, int32_t table_dtype, const float *level_table, uint32_t L,
                             const void *frags, const float *bias, int32_t mlp_dtype, int32_t mlp_in,
                             const float *points, int64_t n, const float *gx, const float *gy, const float *gz,
                             int32_t nx, int32_t ny, int32_t nz, const uint8_t *occ, int32_t occ_n, float *sdf,
                             void *stream) {
    if (!table || !level_table || !frags || !bias || !sdf || L == 0 || L > 16 || mlp_in != (int)L * 2)
        return nof::set_error(NOF_EINVAL, "query_sdf: bad table / MLP arguments (C = 2, L <= 16)");
    if (table_dtype != mlp_dtype) return nof::set_error(NOF_EINVAL, "query_sdf: table and MLP dtypes must match");
    if (!points && (!gx || !gy || !gz || nx <= 0 || ny <= 0 || nz <= 0))
        return nof::set_error(NOF_EINVAL, "query_sdf: need points or three grid axes");
    if (!points) n = (int64_t)nx * ny * nz;
    if (n <= 0) return NOF_OK;
    nof::FieldArgs a{};
    nof::fill_model(a, table, level_table, L, mlp_in, frags, bias);
    nof::QueryArgs q{points, gx, gy, gz, nx, ny, nz, n, occ, occ_n, sdf};
    launch_query_sdf(mlp_dtype == NOF_F16, a, q, (hipStream_t)stream);
    return nof::check_launch("query_sdf");
}

extern "C" int nof_query_field(const void *table, int32_t table_dtype, const float *level_table, uint32_t L,
                               const void *frags, const float *bias, int32_t mlp_dtype, int32_t mlp_in,
                               const float *points, int64_t n, const float *ff, int32_t n_frames, int32_t n_ff,
                               int32_t frame_id, float *sdf, float *grad, float *rgb, void *stream) {
    // every refusal comes before the first HIP call
    if (!sdf && !grad && !rgb) return nof::set_error(NOF_EINVAL, "query_field: no output requested (sdf, grad and rgb are NULL)");
    if (n < 0) return nof::set_error(NOF_EINVAL, "query_field: n=%lld is negative", (long long)n);
    if (!points && n > 0) return nof::set_error(NOF_EINVAL, "query_field: points is NULL with n=%lld", (long long)n);
    if (table_dtype != mlp_dtype || (mlp_dtype != NOF_F16 && mlp_dtype != NOF_F32))
        return nof::set_error(NOF_EINVAL, "query_field: table and MLP dtypes must match (both f16 or both f32)");
    if (L == 0 || L > 16 || mlp_in != (int)L * 2)
        return nof::set_error(NOF_EINVAL, "query_field: needs 1<=L<=16 and C=2 (got L=%u, mlp_in=%d)", L, mlp_in);
    if (!table || !level_table || !frags || !bias)
        return nof::set_error(NOF_EINVAL, "query_field: table / level_table / frags / bias is NULL");
    if (int rc = nof::check_frame_features("query_field", n_ff, ff)) return rc;
    if (ff && n_ff > 0 && (frame_id < 0 || frame_id >= n_frames))
        return nof::set_error(NOF_EINVAL, "query_field: frame_id %d outside the %d frames", frame_id, n_frames);
    if (n == 0) return NOF_OK;
    nof::FieldArgs a{};
    nof::fill_model(a, table, level_table, L, mlp_in, frags, bias);
    hipStream_t st = (hipStream_t)stream;
    const bool amp = mlp_dtype == NOF_F16;
    if (!grad && !rgb) {   // the SDF alone is k_query_sdf's work: its kernel runs it
        nof::QueryArgs q{points, nullptr, nullptr, nullptr, 0, 0, 0, n, nullptr, 0, sdf};
        launch_query_sdf(amp, a, q, st);
        return nof::check_launch("query_field(sdf)");
    }
    const bool with_ff = ff && n_ff > 0;
    nof::QueryFieldArgs q{points, n, with_ff ? ff + (size_t)frame_id * n_ff : nullptr, with_ff ? n_ff : 0, sdf, grad, rgb};
    NOF_LAUNCH_TYPED(amp, nof::k_query_field, dim3(query_blocks(n)), dim3(256),   // amp: + the fp16-rounded bias image
                     (nof::staged_bytes<TM, nof::N_FRAGS>(sizeof(TM) == 2)), st, a, q);
    return nof::check_launch("query_field");
}

namespace {
// the render's workspace: per-ray context records, then the per-tile records
struct RenderWorkspace : nof::Carver {
    float *rctx, *rrec;
    RenderWorkspace(void *base, int R, int S) : Carver(base) {
        rctx = take<float>((size_t)R * nof::RCTX);
        rrec = take<float>((size_t)R * (S / 32) * nof::RREC);
    }
};
}  // namespace

extern "C" size_t nof_render_workspace_bytes(int32_t R, int32_t S) {
    return (R < 0 || S <= 0) ? 0 : RenderWorkspace(nullptr, R, S).bytes;
}

extern "C" int nof_render_rays(const nof_field_desc *d, const nof_render_out *o, void *stream) {
    // every refusal comes before the first HIP call, as in nof_field_step
    if (!d || !o) return nof::set_error(NOF_EINVAL, "render_rays: desc / out is NULL");
    if (d->S <= 0 || d->S % 32 != 0 || d->S > 320 || d->N_oct + d->N_dep != d->S)
        return nof::set_error(NOF_EINVAL, "render_rays: S=%d must be N_oct+N_dep, a multiple of 32, <= 320", d->S);
    if (int rc = nof::check_geometry("render_rays", d, true)) return rc;
    if (!o->rgb) return nof::set_error(NOF_EINVAL, "render_rays: out.rgb is NULL");
    if (!o->depth) return nof::set_error(NOF_EINVAL, "render_rays: out.depth is NULL");
    if (d->R < 0 || (int64_t)d->R * (d->S / 32) > INT32_MAX)
        return nof::set_error(NOF_EINVAL, "render_rays: R=%d (0 <= R, R * S / 32 < 2^31)", d->R);
    if (d->R == 0) return NOF_OK;
    if (d->Kmax <= 0) return nof::set_error(NOF_EINVAL, "render_rays: Kmax=%d", d->Kmax);
    if (!d->rays || !d->tf || !d->intervals || !d->totals)
        return nof::set_error(NOF_EINVAL, "render_rays: rays / tf / intervals / totals is NULL (nof_trace_rays)");
    if (int rc = nof::check_model_pointers("render_rays", d)) return rc;
    if (int rc = nof::check_frame_features("render_rays", d->n_ff, d->ff)) return rc;
    bool amp;
    if (int rc = nof::check_dtype_pair("render_rays", d, amp)) return rc;
    if (!o->workspace) return nof::set_error(NOF_EINVAL, "render_rays: out.workspace is NULL (nof_render_workspace_bytes)");

    nof::FieldArgs a{};
    nof::fill_sampling(a, d);
    nof::fill_model(a, d);
    a.perturb = 0;   // render_images renders with perturb=False: no draws are read
    const RenderWorkspace ws(o->workspace, d->R, d->S);
    a.rctx = ws.rctx;
    const nof::RenderOut ro{o->rgb, o->depth, o->z, o->sdf, o->valid, ws.rrec};

    hipStream_t st = (hipStream_t)stream;
    const int n_cu = nof::cu_count();
    hipLaunchKernelGGL(nof::k_render_ctx, dim3(nof::div_up(a.R, 256)), dim3(256), 0, st, a);
    if (int rc = nof::check_launch("render_rays(ctx)")) return rc;
    // persistent 8-wave blocks: at most 4 per CU (the staged fragments: 30 KB fp16, 54 KB fp32)
    const dim3 grid(nof::tile_blocks((int64_t)a.R * (a.S / 32), nof::RENDER_WPB, n_cu, 4));
    NOF_LAUNCH_TYPED(amp, nof::k_render, grid, dim3(nof::RENDER_WPB * 64),
                     (nof::staged_bytes<TM, nof::RENDER_NFR>(false, nof::RENDER_LVT_BYTES)), st, a, ro);
    if (int rc = nof::check_launch("render_rays(render)")) return rc;
    hipLaunchKernelGGL(nof::k_render_final, dim3(nof::div_up(a.R, 256)), dim3(256), 0, st, a, ro);
    return nof::check_launch("render_rays(final)");
}

namespace {
// the surface render's workspace: per-ray records, the interval lists, the bracket records
struct ViewWorkspace : nof::Carver {
    float *vray, *iv, *brk;
    ViewWorkspace(void *base, int n, int Kmax) : Carver(base) {
        vray = take<float>((size_t)n * nof::VRAY);
        iv = take<float>((size_t)n * Kmax * 2);
        brk = take<float>((size_t)n * nof::VBRK);
    }
};
}  // namespace

extern "C" size_t nof_render_view_workspace_bytes(int32_t n, int32_t Kmax) {
    return (n < 0 || Kmax <= 0) ? 0 : ViewWorkspace(nullptr, n, Kmax).bytes;
}

extern "C" int nof_render_view(const nof_field_desc *d, const nof_view_desc *w, const nof_view_out *o, void *stream) {
    // every refusal comes before the first HIP call, as in nof_render_rays
    if (!d || !w || !o) return nof::set_error(NOF_EINVAL, "render_view: desc / view / out is NULL");
    bool amp;
    if (int rc = nof::check_geometry("render_view", d, true)) return rc;
    if (int rc = nof::check_dtype_pair("render_view", d, amp)) return rc;
    if (int rc = nof::check_model_pointers("render_view", d)) return rc;
    if (int rc = nof::check_frame_features("render_view", d->n_ff, d->ff)) return rc;
    if (d->n_ff > 0 && (w->frame_id < 0 || w->frame_id >= w->n_frames))
        return nof::set_error(NOF_EINVAL, "render_view: frame_id %d outside the %d frames", w->frame_id, w->n_frames);
    if (d->Kmax <= 0) return nof::set_error(NOF_EINVAL, "render_view: Kmax=%d", d->Kmax);
    if (w->H <= 0 || w->W <= 0 || (int64_t)w->H * w->W > INT32_MAX)
        return nof::set_error(NOF_EINVAL, "render_view: bad image size H=%d W=%d", w->H, w->W);
    if (!(w->K[0] != 0.f) || !(w->K[4] != 0.f))
        return nof::set_error(NOF_EINVAL, "render_view: K has a zero focal length (fx=%g fy=%g)", w->K[0], w->K[4]);
    if (w->n < 0 || w->n > (1 << 24)) return nof::set_error(NOF_EINVAL, "render_view: n=%d (0 <= n <= 2^24 rays a call)", w->n);
    if (!w->pixels && (w->pixel0 < 0 || (int64_t)w->pixel0 + w->n > (int64_t)w->H * w->W))
        return nof::set_error(NOF_EINVAL, "render_view: pixels %d..%lld leave the %dx%d image", w->pixel0,
                              (long long)w->pixel0 + w->n, w->H, w->W);
    if (!(w->step > 0.f) || w->max_steps <= 0 || w->max_steps > (1 << 20) || w->n_refine < 0 || w->n_refine > 64)
        return nof::set_error(NOF_EINVAL, "render_view: step=%g (> 0), max_steps=%d (1..2^20), n_refine=%d (0..64)", w->step,
                              w->max_steps, w->n_refine);
    if (!w->occ || w->occ_n <= 0) return nof::set_error(NOF_EINVAL, "render_view: occ is NULL or occ_n=%d", w->occ_n);
    if (w->n == 0) return NOF_OK;
    if (!o->t || !o->depth || !o->normal || !o->rgb || !o->hit)
        return nof::set_error(NOF_EINVAL, "render_view: out.t / depth / normal / rgb / hit is NULL");
    if (!o->workspace)
        return nof::set_error(NOF_EINVAL, "render_view: out.workspace is NULL (nof_render_view_workspace_bytes)");

    nof::FieldArgs a{};
    nof::fill_model(a, d);
    a.n_ff = 0; a.ff = nullptr;   // the one frame's feature row travels in ViewArgs
    const ViewWorkspace ws(o->workspace, w->n, d->Kmax);
    nof::ViewArgs v{};
    for (int i = 0; i < 12; ++i) v.c2w[i] = w->c2w[i];
    v.fx = w->K[0]; v.fy = w->K[4]; v.cx = w->K[2]; v.cy = w->K[5];
    v.W = w->W; v.pixels = w->pixels; v.pixel0 = w->pixel0; v.n = w->n;
    v.step = w->step; v.max_steps = w->max_steps; v.n_refine = w->n_refine;
    v.occ = w->occ; v.N = w->occ_n; v.Kmax = d->Kmax;
    v.n_ff = d->n_ff;
    v.ff = d->n_ff > 0 ? d->ff + (size_t)w->frame_id * d->n_ff : nullptr;
    v.vray = ws.vray; v.iv = ws.iv; v.brk = ws.brk;
    v.t = o->t; v.depth = o->depth; v.normal = o->normal; v.rgb = o->rgb; v.hit = o->hit;
    v.index = o->index; v.tiles = o->tiles;

    hipStream_t st = (hipStream_t)stream;
    const int n_cu = nof::cu_count();
    hipLaunchKernelGGL(nof::k_view_trace, dim3(nof::div_up(v.n, 256)), dim3(256), 0, st, v);
    if (int rc = nof::check_launch("render_view(trace)")) return rc;
    // a wave per ray, 4-wave blocks: persistent from 8 blocks per CU
    const int mblocks = nof::tile_blocks(v.n, 4, n_cu, 8);
    NOF_LAUNCH_TYPED(amp, nof::k_view_march, dim3(mblocks), dim3(256), (nof::staged_bytes<TM, nof::VIEW_NFR>()), st, a, v);
    if (int rc = nof::check_launch("render_view(march)")) return rc;
    const int sblocks = nof::tile_blocks(((int64_t)v.n + 31) / 32, 4, n_cu, 2);
    NOF_LAUNCH_TYPED(amp, nof::k_view_shade, dim3(sblocks), dim3(256),
                     (nof::staged_bytes<TM, nof::N_FRAGS>(sizeof(TM) == 2)), st, a, v);
    return nof::check_launch("render_view(shade)");
}
