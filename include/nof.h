/*
 * nof.h — C ABI of the MI355X-native neural-object-field (NOF) trainer.
 *
 * Every entry point takes plain device pointers, sizes and a HIP stream
 * (hipStream_t passed as void*; NULL = legacy default stream), launches
 * asynchronously on that stream, keeps no state between calls and returns a
 * nof_status. Callers pre-allocate every output (the reference's ownership
 * convention, grid.py:54-59,86-91 / nerf_runner.py:1006). On failure the call
 * returns non-zero and nof_last_error() describes it (the reference raises
 * c10::Error / std::runtime_error -> Python RuntimeError; the Python shims in
 * bundlesdf_amd/ convert a non-zero status into RuntimeError).
 *
 * Group 1 (B1 in SURVEY.md §8b) replaces the reference's torch-extension
 * entry points one-for-one; group 2 is the fused training step the trainer
 * (bundlesdf_amd/nerf_runner.py) drives.
 */
#ifndef NOF_H
#define NOF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    NOF_OK = 0,
    NOF_EINVAL = 1,   /* bad argument (shape / dtype / unsupported C or D) */
    NOF_ELAUNCH = 2,  /* kernel launch failed */
    NOF_EDEVICE = 3   /* device-side error flag raised */
} nof_status;

typedef enum { NOF_F32 = 0, NOF_F16 = 1 } nof_dtype;

#define NOF_MAX_LEVELS 32

/* Thread-local description of the last failure (static storage). */
const char *nof_last_error(void);
/* Library build identification string (arch, build flags). */
const char *nof_version(void);

/* ------------------------------------------------------------------ group 1
 * Drop-in replacements of the reference extension entry points.
 */

/* Replaces gridencoder.grid_encode_forward
 *   (mycuda/torch_ngp_grid_encoder/gridencoder.h:23, gridencoder.cu:447-470).
 * inputs [B,D] f32 in [0,1]; embeddings [sO,C] (dtype); offsets [L+1] i32;
 * outputs [L,B,C] (dtype); dy_dx [B,L*D*C] (dtype) when calc_grad_inputs.
 * C in {1,2,4,8}, D in {1..5}; gridtype 0 = hash, 1 = tiled. */
int nof_grid_encode_forward(const float *inputs, const void *embeddings, const int32_t *offsets, void *outputs,
                            uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                            int calc_grad_inputs, void *dy_dx, uint32_t gridtype, int align_corners,
                            int dtype, void *stream);

/* Replaces gridencoder.grid_encode_backward
 *   (gridencoder.h:24, gridencoder.cu:472-502).
 * grad [L,B,C]; grad_embeddings [sO,C] zero-initialised by the caller;
 * grad_inputs [B,D] (dtype) when calc_grad_inputs. Accumulation into
 * grad_embeddings uses device atomics (order-dependent low bits, as in the
 * reference). */
int nof_grid_encode_backward(const void *grad, const float *inputs, const void *embeddings,
                             const int32_t *offsets, void *grad_embeddings, uint32_t B, uint32_t D, uint32_t C,
                             uint32_t L, float S, uint32_t H, int calc_grad_inputs, const void *dy_dx,
                             void *grad_inputs, uint32_t gridtype, int align_corners, int dtype, void *stream);

/* Replaces common.sampleRaysUniformOccupiedVoxels (mycuda/common.h:28,
 * common.cu:107-125). z_in_out [N,K,2], z_sampled [N,S], z_vals [N,S] f32.
 * Malformed rays (the reference prints and spins forever, common.cu:66-71,
 * 87-92) leave z unchanged and increment *error_count (device int, may be
 * NULL). */
int nof_sample_rays_uniform_occupied_voxels(const float *z_in_out, const float *z_sampled, float *z_vals,
                                            int32_t n_rays, int32_t n_intersect, int32_t n_samples,
                                            int32_t *error_count, void *stream);

/* Replaces common.postprocessOctreeRayTracing (common.h:29, common.cu:151-167).
 * out [n_rays, max_intersections, 2] f32 must be zeroed by the caller (the
 * reference allocates it itself, on cuda:0 — common.cu:158; the Python shim
 * allocates on the input's device). */
int nof_postprocess_octree_ray_tracing(const int64_t *ray_index, const float *depth_in_out,
                                       const int64_t *unique_intersect_ray_ids, const int64_t *start_poss,
                                       int64_t n_hits, int64_t n_unique, int32_t max_intersections,
                                       float *out, void *stream);

/* Replaces common.rayColorToTextureImageCUDA (common.h:30, common.cu:188-238):
 * barycentric UV of each hit point. F [Fc,3] i64, V [Nv,3] f32,
 * hit_locations [M,3] f32, hit_face_ids [M] i64, uvs_tex [Nv,2] f32,
 * uvs [M,2] f32 (output). */
int nof_ray_color_to_texture_uv(const int64_t *F, const float *V, const float *hit_locations,
                                const int64_t *hit_face_ids, const float *uvs_tex, float *uvs, int64_t n_hits,
                                void *stream);

/* ------------------------------------------------------------------ group 2
 * Fused training step (bundlesdf_amd/nerf_runner.py). Replaces the per-step
 * work of NerfRunner.train_loop (nerf_runner.py:677-762): kaolin ray trace
 * (Utils.py:443-475), the two samplers (nerf_runner.py:979-1080), run_network
 * (:1226-1303), raw2outputs (:1131-1168), the losses (nerf_helpers.py:367-399)
 * and their backward, and Adam.
 */

/* Per-level float32 scale and resolution exactly as gridencoder.cu:155-156
 * computes them (host function, no device work). */
void nof_level_params(uint32_t L, float S, uint32_t H, float *scales, uint32_t *resolutions);

/* Dense-occupancy ray trace at grid resolution N over [-1,1]^3 (replaces
 * kaolin unbatched_raytrace + postprocessOctreeRayTracing, Utils.py:457-470).
 * occ [N^3] u8 (x fastest); rays_o/rays_d [R,3] f32 world (unit d);
 * out [R,Kmax,2] f32 (zero-padded), counts [R] i32 (may be NULL). */
int nof_octree_ray_trace(const uint8_t *occ, int32_t N, const float *rays_o, const float *rays_d, int32_t R,
                         int32_t Kmax, float *out, int32_t *counts, void *stream);

/* Per-step schedule on the device (hipGraph replay). The step's scalars — the
 * truncation band of get_truncation (nerf_runner.py:661-674), the learning rates
 * of schedule_lr (:577-581, applied every 10 steps, :761-762) and the sampling
 * seeds — are functions of the global step. nof_step_schedule reads the device
 * step counter *step, writes the block for that step into *out and advances
 * *step, all on `stream`; the consumers below take the block by device pointer
 * (nullable: NULL = use their scalar arguments), so one captured graph replays
 * every step with the schedule of the step it runs as. */
typedef struct {
    double lr0, lr1;          /* Adam learning rates of group 0 (table + MLP + features) / group 1 (poses) */
    float trunc;              /* truncation * sc_factor */
    uint32_t seed;            /* field-pass sampling seed: step * 0x9E3779B1 + seed_base */
    uint32_t batch_seed;      /* nof_sample_batch seed: batch_seed_base + step */
    int32_t step;             /* the global step this block belongs to */
} nof_step_params;

typedef struct {
    double lrate, lrate_pose, decay_rate;   /* cfg lrate, lrate_pose, decay_rate */
    double trunc, trunc_start, sc_factor;   /* cfg trunc, trunc_start, sc_factor */
    int32_t trunc_decay;      /* 0: constant, 1: 'linear', 2: 'exp' (cfg trunc_decay_type) */
    int32_t n_step;           /* cfg n_step */
    uint32_t seed_base, batch_seed_base;
} nof_schedule_desc;

int nof_step_schedule(const nof_schedule_desc *d, int32_t *step, nof_step_params *out, void *stream);

/* Step 1 — batch gather + ray setup + ray trace + interval clipping
 * (render_rays :1043-1059, Utils.py:443-475, sample_rays_uniform_occupied_voxels
 * :984-1001). pool [N_pool,12] f32 ray table (reference column order); ids [R]
 * (NULL: the first R rows of pool are the batch); tf [F,16] world_from_cam per
 * frame (pose correction applied); rays_out [R,12] (written when ids != NULL);
 * intervals [R,Kmax,2] f32 in z units: the ray's counts[r] intervals, then (when counts[r] <
 * Kmax) one zero entry ending the list — the entries after it are not written; totals [R];
 * counts [R] (nullable). */
int nof_trace_rays(const float *pool, const int32_t *ids, int32_t R, const float *tf, const uint8_t *occ, int32_t N,
                   int32_t Kmax, float near_sc, float far_sc, float trunc, float *rays_out, float *intervals,
                   float *totals, int32_t *counts, const nof_step_params *sp, void *stream);

/* nof_trace_rays on the step's batch of an epoch permutation (NerfRunner's DataLoader,
 * nerf_runner.py:90-107: consecutive R-id slices of one randperm): ids = perm + (sp->step -
 * *epoch_step0) * R, where *epoch_step0 (device int) is the global step that drew the epoch's first
 * slice. Both are read on the device, so one captured graph replays every step of an epoch with no
 * per-step id copy; the caller rewrites perm (same buffer) and *epoch_step0 only when a new epoch
 * starts. sp and epoch_step0 must not be NULL. The caller keeps (step - *epoch_step0 + 1) R <= the
 * permutation's length. */
int nof_trace_rays_epoch(const float *pool, const int32_t *perm, const int32_t *epoch_step0, int32_t R,
                         const float *tf, const uint8_t *occ, int32_t N, int32_t Kmax, float near_sc, float far_sc,
                         float trunc, float *rays_out, float *intervals, float *totals, int32_t *counts,
                         const nof_step_params *sp, void *stream);

/* Throughput-mode ray selection: rays_per_frame uniform draws (with replacement)
 * inside each frame's contiguous pool segment [frame_start[f], frame_start[f+1]),
 * written per frame in ascending pool order (rays_per_frame <= 4096). */
int nof_sample_batch(const int64_t *frame_start, int32_t F, int32_t rays_per_frame, uint32_t seed, int32_t *ids,
                     const nof_step_params *sp, void *stream);

/* Packs the NeRFSmall parameters (flat, MLP_KEYS order, 9107 f32) into MFMA
 * A-operand fragments (frags, mlp_dtype) and a [5][64] bias image using the
 * index table of bundlesdf_amd/mlp_layout.py. */
int nof_pack_mlp(const float *mlp, const int32_t *idx, int32_t n_frag_elems, int32_t n_bias, void *frags,
                 float *bias, int mlp_dtype, void *stream);

/* Step 2 — the fused field pass: sampling, encode, MLP (MFMA), compositing,
 * losses and the full backward. Accumulates (does not zero) grad_table and
 * grad_mlp; zeroes loss_acc [144] and then writes it; writes ray_grad [R,12] =
 * dL/d tf[frame][0:3,0:4] per ray. All gradients are multiplied by *loss_scale
 * (GradScaler). The struct has no padding (its 4-byte fields come in pairs between the
 * pointers), so any field added or removed changes nof_field_desc_size(). */
typedef struct {
    /* ---- batch inputs and scalars */
    const float *rays;        /* [R,12] */
    const float *tf;          /* [F,16] */
    const float *intervals;   /* [R,Kmax,2] */
    const float *totals;      /* [R] */
    const float *t_rand;      /* [R,S] stratification draws, or NULL (counter RNG from seed) */
    uint32_t seed;
    int32_t R, Kmax, N_oct, N_dep, S, perturb;
    float near_sc, far_sc, trunc, neg_trunc_ratio, sdf_lambda, fs_sdf, first_frame_weight;
    float rgb_weight, fs_weight, empty_weight, trunc_weight;
    float fs_rgb_weight;      /* cfg fs_rgb_weight (train_loop :728-731): 0 = off; > 0 adds
                                 fs_rgb_weight * mean(((sigmoid(rgb logits) - 1) * front)^2 * sample_weights),
                                 the unweighted mean in loss_acc[140] */
    int32_t skip_pose_grad;   /* 1: poses frozen (cfg optimize_poses = 0): no dL/dtf — the reference's grid
                                 backward then skips dy_dx (inputs need no grad), so k_scatter skips the
                                 corner re-gather and ray_grad is not written */
    const float *loss_scale;  /* device scalar */
    const nof_step_params *step_params;   /* device, nullable: trunc and seed from the block (graph replay) */
    /* ---- parameters */
    const void *table;        /* [T,2] table_dtype (the fp16 mirror under amp) */
    const float *levels;      /* [L,4] from nof_level_table: scale, res, row offset, rows (int bits) */
    uint32_t L, C, D;
    int32_t table_dtype, mlp_dtype;
    int32_t n_ff;             /* cfg frame_features (0..3): FeatureArray channels fed to the colour net
                                 (nerf_runner.py:221,234-235,1268-1277); 0 = none */
    const void *frags;        /* nof_pack_mlp output */
    const float *bias;
    const float *ff;          /* [F, n_ff] f32 FeatureArray.data, or NULL */
    /* ---- outputs */
    float *grad_table;        /* [T,2] f32 (fp32 mode) */
    void *grad_table16;       /* [T,2] f16 (amp mode: packed fp16x2 atomics, as the reference's __half2 path) */
    float *grad_mlp;          /* [9107 + 64*n_ff] f32 (mlp_layout.offsets) */
    float *grad_ff;           /* [F, n_ff] f32 gradient (accumulated, scaled by *loss_scale), or NULL */
    float *ray_grad;          /* [R,12] f32 */
    float *loss_acc;          /* [144] f32: rgb, fs (free space), empty, sdf — normalised, unscaled;
                                 [4] samples inside the box, [5] samples through the backward, [6..7] not written
                                 (FusedStep puts reg_features in [6] when frame_features > 0,
                                 pose_reg in [7] when pose_reg_weight > 0);
                                 [8 + 2i], [9 + 2i] (i < 64): HBM scatter atomics (table flush,
                                 probe overflow), spread over 64 counters — sum them (count_atomics);
                                 [136..139] executed tiles: sigma net, colour net, colour / sigma-only
                                 backward records; [140] fs_rgb loss (the reference's unweighted metric,
                                 train_loop :730; the loss adds fs_rgb_weight times it); [141..143] not written */
    /* ---- debug outputs */
    float *dbg_z;             /* optional [R,S] */
    float *dbg_raw;           /* optional [R,S,4] (rgb logits, sdf) */
    uint8_t *dbg_valid;       /* optional [R,S] */
    float *dbg_rgb;           /* optional [R,3] */
    /* ---- workspace: caller-owned scratch the step rewrites */
    void *workspace;          /* nof_field_workspace_bytes(R, S, mlp_dtype) bytes */
    void *table_quads;        /* amp, optional (NULL: unused): 16 B per table row (n_rows = the last level's
                                 offset + size), rebuilt from `table` at the start of every field pass with
                                 R >= quads_min_rays; row r of a dense level holds the fp16 pairs of rows
                                 {r, r+1, r+rs, r+rs+1} (rs = res + 1), so k_encode reads a cell's 8
                                 corners in two 16-B loads (z, z+1) instead of four 8-B pair loads */
    int64_t table_rows;       /* rows of `table` (= table_quads' length in 16-B records) */
    int32_t quads_prebuilt;   /* 1: the caller rebuilt table_quads for this step with nof_quad_mirror (same
                                 descriptor), ordered before this call (e.g. on a side stream joined by an
                                 event, overlapping the prologue and trace); 0: nof_field_step rebuilds it */
    /* ---- shape knobs: launch shapes and diagnostics, 0 = the library's choice */
    int32_t count_atomics;    /* 1: the scatter kernels count their HBM atomics (table flush, probe overflow) into
                                 loss_acc[8..135] (diagnostics); 0: those words stay zero */
    int32_t ablate;           /* timing-only ablation bits; must be 0 (results are wrong otherwise) */
    int32_t scatter_slots;   /* LDS hash slots per wave for the table-gradient scatter (0 -> 512; power of two, 64..2048) */
    int32_t scatter_levels_per_wave; /* 0: by batch size (a wave per ray from 192 K rays, 8 levels
                                        per wave from 48 K, 4 from 8 K, else 2); n: scatter waves take
                                        n levels of a ray */
    int32_t bwd_flush;        /* amp MLP backward weight-gradient flush: 0 / 2 (default) summed over the 8-wave
                                 block first (one atomic per element per block), 1 one atomic per element per wave */
    int32_t compact_per_block; /* k_compact flags per block: 0 by batch size (4096 from 262,144 tiles, where each
                                  thread reads 16 flags with one 16-B load; else 512), or a multiple of 256 in
                                  [256, 4096] — the tests force 4096 on small batches to run the 16-flag path */
    int32_t encode_group;     /* k_encode levels whose corner gathers a lane keeps in flight together: 0 by batch
                                 size (1 from 8,192 rays, where 8 waves per SIMD hide the gathers; more below,
                                 where the grid is too small to), or 1, 2, 4 */
    int32_t quads_min_rays;   /* batch size from which table_quads is used (0 -> 32768, the measured break-even
                                 of its per-step rebuild); tests lower it to run the headline's quad encode on
                                 oracle-sized batches */
    int32_t xcd_order;        /* bit 0: k_encode, bit 1: k_scatter take their blocks in XCD-contiguous order
                                 (each XCD's L2 serves a contiguous range of the batch); 0: dispatch order */
} nof_field_desc;

/* Launches on `stream`: k_ray_ctx (one 128-B context record per ray: direction,
 * target, pose rows, view direction, depth, interval total, frame), [k_quad_mirror
 * (amp, large batches)], k_encode (one wave per 32-sample tile: sampling +
 * multires encode + sigma net on MFMA, sdf-loss terms; flags the tiles whose
 * backward is non-zero and hands them per-sample loss terms through the
 * workspace), k_compact (lists of the backward and colour tiles), k_colour
 * (persistent waves over the colour tiles: colour net on MFMA), k_ray_final (a
 * thread per ray: compositing, losses), k_mlp_bwd (two persistent passes over
 * the backward list: MFMA MLP backward with the weight / bias gradients
 * accumulated in registers, and dL/dfeature; amp takes the weight gradients'
 * K = samples operands from LDS transposes), k_scatter (a wave per (ray, level
 * group): table-gradient scatter + input gradient). */
int nof_field_step(const nof_field_desc *desc, void *stream);

/* sizeof(nof_field_desc) of the build that made this library: a binder compares it with its own
 * mirror of the struct right after loading, before any call that takes a descriptor (a library
 * built from another header would read its pointers from the wrong offsets). */
size_t nof_field_desc_size(void);

/* The xy-quad mirror rebuild of nof_field_step (table -> table_quads), as its own launch: reads
 * table, levels, L, C, R, table_quads, table_rows, quads_min_rays and the dtypes of desc; a no-op
 * when the step would not use the mirror. Lets the caller overlap it with the work before the
 * field pass (the step then runs with quads_prebuilt = 1). No reference counterpart: the quad
 * mirror is this library's layout for the encode's corner gathers (gridencoder.cu:145-205). */
int nof_quad_mirror(const nof_field_desc *desc, void *stream);

/* Forward-only ray render (replaces what NerfRunner.render_images, nerf_runner.py:584-634, takes
 * from render() with perturb=False: render_rays :1043-1087, raw2outputs :1131-1168 and the depth
 * rule of :602-610). Outputs of nof_render_rays; z / sdf / valid are optional (NULL: nothing per
 * sample is written to memory). */
typedef struct {
    float *rgb;        /* [R,3] depth-guided composite of the sigmoid colours: sum over valid samples of
                          w sigmoid(rgb logits) / (sum over all samples of w + 1e-10), w the bell weight of
                          raw2outputs (0 for rays with depth > far) */
    float *depth;      /* [R] signs[i] = sdf[i+1] * sdf[i] (float32) over the ray's S samples in the
                          reference's order (N_oct octree samples, then N_dep around-depth samples, unsorted):
                          far_sc when every signs[i] > 0, else z[j], j the first i with signs[i] < 0 (j = 0
                          when there is none) — computed from the z / sdf values this call returns */
    float *z;          /* optional [R,S] sample z */
    float *sdf;        /* optional [R,S] sigma-net output; samples outside [-1,1]^3 carry the net's output on
                          a zero encoding (run_network :1246,1265) */
    uint8_t *valid;    /* optional [R,S] 1 = inside [-1,1]^3 */
    void *workspace;   /* nof_render_workspace_bytes(R, S) bytes of scratch (per-ray context records,
                          one 48-B record per 32-sample tile) */
} nof_render_out;

size_t nof_render_workspace_bytes(int32_t R, int32_t S);

/* Reads of desc: rays, tf, intervals, totals (nof_trace_rays output), R, Kmax, N_oct, N_dep, S,
 * near_sc, far_sc, trunc, neg_trunc_ratio, sdf_lambda, table, levels, L, C, D, the dtypes, n_ff, ff,
 * frags, bias. Everything else is ignored: sampling is unperturbed (no t_rand, no seed), the pair
 * table is read (never table_quads), no gradient, loss or workspace field is touched. Launches
 * k_render_ctx (a thread per ray), k_render (a wave per 32-sample tile: sampling, encode, sigma net,
 * colour net where a valid sample has weight) and k_render_final (a thread per ray sums its tiles in
 * order and applies the depth rule): no atomics, so two calls on the same inputs are bit-identical.
 * The descriptor is validated before the first HIP call; R == 0 returns NOF_OK with no launch. */
int nof_render_rays(const nof_field_desc *desc, const nof_render_out *out, void *stream);

/* SDF query (replaces run_network_density, nerf_runner.py:1306-1346, as used
 * by extract_mesh :1349-1382): clip to [-1,1], multires encode, sigma net.
 * Point mode: points [n,3] f32. Grid mode (points NULL): the nx*ny*nz points
 * (gx[i], gy[j], gz[k]) in meshgrid 'ij' order. occ [occ_n^3] u8 (x fastest,
 * nullable): points in empty voxels read 1.0, as extract_mesh fills them.
 * table / level_table / frags / bias as for nof_field_step (amp: fp16 table
 * mirror + fp16 fragments). sdf [n] f32 output. */
int nof_query_sdf(const void *table, int32_t table_dtype, const float *level_table, uint32_t L, const void *frags,
                  const float *bias, int32_t mlp_dtype, int32_t mlp_in, const float *points, int64_t n,
                  const float *gx, const float *gy, const float *gz, int32_t nx, int32_t ny, int32_t nz,
                  const uint8_t *occ, int32_t occ_n, float *sdf, void *stream);

/* Field point query: SDF, its gradient with respect to the point, and colour at points [n,3] f32
 * (run_network_density(get_normals=True), nerf_runner.py:1306-1346, and run_network as
 * mesh_vertex_color_from_network calls it, :1411-1428). table / table_dtype / level_table / L / frags /
 * bias / mlp_dtype / mlp_in as for nof_query_sdf (the gradient reads the backward fragments FR_B2 /
 * FR_B1 that nof_pack_mlp already packs). Outputs, each nullable, at least one set:
 *   sdf  [n]   f32: bit-identical to nof_query_sdf on the same points (clip to [-1,1]);
 *   grad [n,3] f32: d sdf / d point at the CLIPPED point (the reference's autograd leaf is the clipped
 *                   tensor: a point outside the box gets the gradient at its clipped position); amp
 *                   rounds where the reference's autograd rounds (fp16 dy_dx, fp16 Linear backward
 *                   results, fp16 input-backward sums in level order);
 *   rgb  [n,3] f32: sigmoid of the colour net at view direction (0,0,0) with the frame features of
 *                   frame_id (ff [n_frames, n_ff] f32, NULL / n_ff 0 for a model without). Validity is
 *                   run_network's: a point with any |x| > 1 is NOT clipped, its grid embedding is zero
 *                   (:1244-1265) — unlike sdf / grad of the same call.
 * Every argument is validated before the first HIP call; n == 0 returns NOF_OK with no launch. No
 * atomics, nothing written but the outputs. With sdf alone the launch is nof_query_sdf's kernel. */
int nof_query_field(const void *table, int32_t table_dtype, const float *level_table, uint32_t L, const void *frags,
                    const float *bias, int32_t mlp_dtype, int32_t mlp_in, const float *points, int64_t n,
                    const float *ff, int32_t n_frames, int32_t n_ff, int32_t frame_id, float *sdf, float *grad,
                    float *rgb, void *stream);

/* Free-camera surface render: depth, normal and colour of the field's zero level set seen from any
 * camera (no pool ray, no frame depth; no reference counterpart — the reference renders an extracted
 * mesh with pyrender, offscreen_renderer.py). Per pixel, fp32 with every operation rounded on its own:
 *   ray      dir_cam = ((u - cx) / fx, -((v - cy) / fy), -1), v^ = dir_cam / |dir_cam|, o = c2w[:3,3],
 *            d = R v^ (the pool's convention; no pose-array correction);
 *   trace    the dense-occupancy DDA of nof_octree_ray_trace over occ, at most Kmax intervals, each
 *            entry clamped to t >= 0; T = their summed length; no interval: a miss;
 *   march    step_eff = max(step, T / max_steps), n = ceil(T / step_eff) samples at occupied length
 *            (k + 0.5) step_eff, mapped to t_k by the occupied-voxel sampler's interval walk (a length
 *            past the walk reads the last exit); SDF as nof_query_sdf (the same bits), front to back;
 *   crossing the first k with sdf_k <= 0: k = 0 gives t* = t_0, else the bracket [t_{k-1}, t_k]; none:
 *            a miss;
 *   refine   n_refine bisections (midpoint 0.5 (lo + hi), keeping sdf_lo > 0 >= sdf_hi), then
 *            t* = lo + (hi - lo) sdf_lo / (sdf_lo - sdf_hi);
 *   outputs  at x* = o + t* d. */
typedef struct {
    float c2w[16];          /* camera-to-world, row-major, normalised space (NerfRunner.poses) */
    float K[9];             /* intrinsics, row-major */
    int32_t H, W;
    const int32_t *pixels;  /* device, optional [n]: row-major pixel index v W + u of each ray; the caller keeps
                               every index in [0, H W) */
    int32_t n;              /* rays of this call (<= 2^24) */
    int32_t pixel0;         /* pixels NULL: ray i is pixel pixel0 + i, pixel0 + n <= H W */
    float step;             /* coarse step along the occupied length (> 0), normalised units */
    int32_t max_steps;      /* upper bound of samples per ray: the step widens to T / max_steps */
    int32_t n_refine;       /* bisection steps on the bracket (0..64) */
    int32_t frame_id;       /* the frame whose features feed the colour net (desc n_ff > 0) */
    int32_t n_frames;       /* rows of desc->ff */
    int32_t occ_n;
    const uint8_t *occ;     /* device [occ_n^3] occupancy, x fastest (as nof_trace_rays) */
} nof_view_desc;

typedef struct {
    float *t;          /* [n] ray parameter of the hit (distance along the unit direction), 0 on a miss */
    float *depth;      /* [n] t |v^_z|: z-depth in normalised units, as depth images / pool column 6 */
    float *normal;     /* [n,3] nof_query_field's gradient at x* over its norm (a zero gradient stays zero) */
    float *rgb;        /* [n,3] sigmoid of the colour net on x*'s geometry features, sh3(d) and the frame's
                          features, with nof_query_field's colour pass */
    uint8_t *hit;      /* [n] 1 on a hit; a miss writes zeros everywhere */
    int32_t *index;    /* optional [n]: the coarse sample k of the crossing, -1 on a miss */
    int32_t *tiles;    /* optional [n]: 32-sample tiles the march evaluated */
    void *workspace;   /* nof_render_view_workspace_bytes(n, desc->Kmax) bytes of scratch */
} nof_view_out;

size_t nof_render_view_workspace_bytes(int32_t n, int32_t Kmax);

/* Reads of desc: Kmax, table, levels, L, C, D, the dtypes, n_ff, ff, frags, bias; everything else is
 * ignored. Launches k_view_trace (a thread per ray: ray, DDA, interval list), k_view_march (a wave per
 * ray over its 32-sample tiles, stopping at the first crossing) and k_view_shade (a wave per 32 rays:
 * bisection, gradient, colour net). No atomics: two calls on the same inputs are bit-identical, and a
 * ray's result does not depend on the rays rendered with it. Everything is validated before the first
 * HIP call; n == 0 returns NOF_OK with no launch. */
int nof_render_view(const nof_field_desc *desc, const nof_view_desc *view, const nof_view_out *out, void *stream);

/* Pose corrections on the device (replaces PoseArray.get_matrices,
 * nerf_helpers.py:127-154, and tf = T @ c2w, nerf_runner.py:1050-1052, with
 * their autograd). data [F,6] f32 (PoseArray.data); c2w [F,4,4] f32;
 * max_rot_rad = max_rot * pi / 180. Writes tf_out [F,4,4] and the Jacobian
 * jac [F,12,6] of tf[:3,:4] w.r.t. data (frame 0 is the identity, zero
 * Jacobian). */
int nof_pose_forward(const float *data, const float *c2w, int32_t F, float max_trans, float max_rot_rad,
                     float *tf_out, float *jac, void *stream);

/* The step prologue in one launch: nof_step_schedule (sched nullable: skipped), nof_pose_forward
 * and nof_pack_mlp with the same arguments and results (graph replay: one kernel node instead of
 * three). */
int nof_step_prologue(const nof_schedule_desc *sched, int32_t *step, nof_step_params *sp_out, const float *data,
                      const float *c2w, int32_t F, float max_trans, float max_rot_rad, float *tf_out, float *jac,
                      const float *mlp, const int32_t *idx, int32_t n_frag_elems, int32_t n_bias, void *frags,
                      float *bias, int mlp_dtype, void *stream);

/* Pose gradient: fg[F,12] (scratch: zero on entry, left zero) = per-frame sum of
 * ray_grad [R,12] over the rays' frame ids (rays [R,12], column 8); grad_pose [F,6]
 * += jac^T fg. F <= 1024. R = 0 (an empty batch: ray_grad / rays may be null) adds nothing. */
int nof_pose_backward(const float *ray_grad, const float *rays, int32_t R, const float *jac, int32_t F, float *fg,
                      float *grad_pose, void *stream);

/* Workspace bytes nof_field_step needs (features, feature gradients, z, tile
 * flags, the backward tile list, per-ray / per-tile hand-off records, per-ray
 * context records). */
size_t nof_field_workspace_bytes(int32_t R, int32_t S, int32_t mlp_dtype);

/* Byte offsets of the workspace sections, in this order: feat, dfeat, zbuf, tile_bwd (tile
 * flags), tile_sid (backward tile list), n_tiles (list counters + loss rows), ray_aux, tile_aux,
 * rctx, gmask, rrec, ctile (colour tile list), and the total (= nof_field_workspace_bytes) —
 * NOF_WS_SECTIONS values into offsets[n]. For host readers of the tile lists / counters. */
#define NOF_WS_SECTIONS 13
int nof_field_workspace_offsets(int32_t R, int32_t S, int32_t mlp_dtype, uint64_t *offsets, int32_t n);

/* Per-kernel timing of nof_field_step: when enabled, every call records HIP
 * events on its stream around its 4 kernels (encode, mlp, scatter, dw).
 * collect synchronises, writes the summed milliseconds per kernel over the
 * recorded calls (n >= 4) and the number of calls, and resets. */
int nof_field_timing(int32_t enable);
int nof_field_timing_collect(float *ms_sum, int32_t n, int32_t *calls);

/* Host helper: fills the [L,4] level table nof_field_step reads (float32
 * scale/resolution of gridencoder.cu:155-156; offsets from the host copy of
 * the GridEncoder offsets buffer). */
void nof_level_table(uint32_t L, float S, uint32_t H, const int32_t *offsets_host, float *table_host);

/* GradScaler.unscale_ + found-inf check over grads [n] (in place); also
 * checks (without modifying) the fp16 table gradient grads16 [n16]. Entries
 * [f16_lo, f16_hi) of grads are gradients the reference holds in fp16 under
 * autocast (nn.Linear weights / biases): a scaled value beyond the fp16 range
 * (|g| >= 65520) counts as an overflow there, as it would in the reference. */
int nof_unscale_check(float *grads, int64_t n, const float *scale, int32_t *found_inf, const void *grads16,
                      int64_t n16, int64_t f16_lo, int64_t f16_hi, void *stream);

/* Adam over the flat buffer; elements >= group1_start use lr1 (pose group),
 * the rest lr0. t = *step_count + 1 (device counter: steps the GradScaler
 * skipped do not count, as in torch). Zeroes grads; the update is skipped
 * (the zeroing is not) when *found_inf. When mirror_f16 != NULL the first
 * mirror_n updated params are also written as fp16 (amp table mirror) and
 * their gradients are read from grads16 (fp16, still scaled: multiplied by
 * 1 / *scale here) instead of grads. sp (nullable): lr0 / lr1 from the step block.
 * active (nullable, nof_adam_active_bytes(n) bytes, zeroed with the moments): one flag per
 * group of 256 consecutive parameters, set once the group had a non-zero gradient; a group
 * that never had one (m = v = 0) is left exactly as dense Adam leaves it — unchanged —
 * without reading or writing its params / moments. Flags must be 1 for any group whose
 * moments were set from outside (0 only where exp_avg = exp_avg_sq = 0). */
size_t nof_adam_active_bytes(int64_t n);
int nof_adam_step(float *params, float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, int64_t group1_start,
                  double lr0, double lr1, float beta1, float beta2, float eps, const int32_t *step_count,
                  const int32_t *found_inf, void *mirror_f16, int64_t mirror_n, void *grads16, const float *scale,
                  const nof_step_params *sp, uint8_t *active, void *stream);

/* GradScaler.update (growth_factor 2, backoff 0.5, interval 2000 in the
 * reference) when enabled; always advances *step_count unless *found_inf,
 * then clears *found_inf. */
int nof_scaler_update(float *scale, int32_t *growth_tracker, int32_t *found_inf, int32_t *step_count,
                      float growth_factor, float backoff_factor, int32_t growth_interval, int enabled, void *stream);

/* Data-parallel exchange (amp): grads[i] = (float)grads16[i], grads16[i] = 0
 * for i < n, so the table gradient joins the flat fp32 all-reduce bucket
 *  instead of being summed in fp16. */
int nof_grad16_to_f32(void *grads16, float *grads, int64_t n, void *stream);

/* fp32 -> fp16 copy (table mirror initialisation). */
int nof_to_half(const float *src, void *dst, int64_t n, void *stream);

/* ------------------------------------------------------------------ group 3
 * Ray-pool construction. Replaces the host loop of
 * NerfRunner.make_frame_rays (nerf_runner.py:244-314) + compute_near_far_and_
 * filter_rays (:39-65) + ray_box_intersection_batch (nerf_helpers.py:403-446)
 * + the octree filter (:300-312) + the octree-cloud denoise (:175-194 in
 * __init__, :408-423 in add_new_frames) for a batch of consecutive frames.
 */
typedef struct {
    const float *rgb;           /* [F,H,W,3] f32 in [0,1] */
    const float *depth;         /* [F,H,W] f32 (sc-scaled; BAD_DEPTH*sc where invalid) */
    const uint8_t *mask;        /* [F,H,W] u8 (object mask, > 0 = object) */
    const uint8_t *occ_mask;    /* [F,H,W] u8 or NULL (> 0 = occluded: removed after dilation) */
    const double *cam_in_world; /* [F,4,4] f64 row-major, normalised GL camera-to-object poses */
    int32_t F, H, W;
    int32_t first_frame_id;     /* global id of frame 0 of the batch (column 8 = first_frame_id + f) */
    int32_t dilate_first;       /* mask dilation kernel of global frame 0 (100) */
    int32_t dilate_other;       /* of the other frames (60 // down_scale_ratio) */
    float fx, fy, cx, cy;       /* intrinsics (of the down-scaled frames), rounded to f32 */
    float near_sc, far_sc;      /* cfg near*sc_factor, far*sc_factor rounded to f32 (invalid-depth test) */
    double far_sc64;            /* far*sc_factor in f64 (denoise candidate test, on float64 rays) */
    double bbox[6];             /* cfg bounding_box: xyz min, xyz max */
    const uint8_t *occ;         /* [n^3] u8 occupancy at the ray-tracing level (x fastest), NULL = no octree filter */
    int32_t occ_n;
    /* denoise point grid from nof_point_grid_build, cell_start NULL = no denoise */
    const int32_t *cell_start;  /* [cells+1] */
    const double *cell_points;  /* [M,3] f64, grouped by cell */
    double grid_origin[3];
    int32_t grid_dims[3];
    double grid_cell;           /* cell edge; must be >= grid_radius */
    double grid_radius;         /* 0.02 * sc_factor: rays whose depth point is farther from every cloud point are dropped */
    void *workspace;            /* nof_ray_pool_workspace_bytes(F, H, W) bytes */
    float *rays;                /* [F*H*W, 12] f32 output (reference column order), first *n_out rows valid */
    int64_t *n_out;             /* device int64: number of rays written */
} nof_ray_pool_desc;

size_t nof_ray_pool_workspace_bytes(int32_t F, int32_t H, int32_t W);

/* Five launches: row / column mask dilation, per-pixel selection (+ near/far,
 * octree trace, denoise radius test), block-offset scan, ordered compaction.
 * Output rows are in the reference's order (frame-major, then row-major
 * pixels). W <= 4096, H <= 1024. */
int nof_make_frame_rays(const nof_ray_pool_desc *desc, void *stream);

/* Uniform grid of the octree point cloud for the denoise radius test:
 * points [M,3] f64 -> cell_start [cells+1] i32, cell_points [M,3] f64 grouped
 * by cell (cell = clamp(floor((p - origin) / cell), 0, dims-1), x fastest),
 * cell_ids [M] i32 (nullable): input index of each grouped point (the order
 * within a cell is unspecified). workspace: nof_point_grid_workspace_bytes(cells). */
size_t nof_point_grid_workspace_bytes(int64_t n_cells);
int nof_point_grid_build(const double *points, int32_t M, const double *origin, const int32_t *dims, double cell,
                         int32_t *cell_start, double *cell_points, int32_t *cell_ids, void *workspace, void *stream);

/* ------------------------------------------------------------------ group 4
 * Scene-bounds / hand-off point-cloud operators, the
 * device replacements of the open3d / sklearn calls in tool.py:18-39,42-63
 * (compute_scene_bounds_worker, find_biggest_cluster) and bundlesdf.py:160-169.
 */

/* remove_statistical_outlier's per-point statistic (open3d PointCloud::
 * RemoveStatisticalOutliers): mean Euclidean distance to the min(k, n)
 * nearest points, the point itself included (exact selection, f64). */
int nof_knn_mean_dist(const double *points, int32_t n, int32_t k, double *mean_dist, void *stream);

/* DBSCAN (sklearn.cluster.DBSCAN, euclidean, neighbourhoods |p - q| <= eps
 * including p; core = neighbourhood size >= min_samples). labels [n] i32:
 * for points of a cluster the lowest core-point index of the cluster (the
 * point sklearn starts that cluster from), -1 for noise; a border point takes
 * the cluster of its lowest-index core neighbour. Uniform grid of cell eps
 * over the points' bounds (origin, dims: cells per axis, <= 2^26 in total).
 * Synchronises `stream` once per union-find round (few rounds). */
size_t nof_dbscan_workspace_bytes(int32_t n, int64_t n_cells);
/* Voxel down-sampling's averaging (open3d VoxelDownSample, AccumulatedPoint):
 * out[s, :] = mean of vals[perm[i], :] for i in [seg_start[s], seg_start[s+1]),
 * summed in that order in f64. vals [M,C], perm [M] i64 (points sorted by
 * voxel, stable), seg_start [S+1] i64, out [S,C]. */
int nof_segment_mean(const double *vals, int32_t C, const int64_t *perm, const int64_t *seg_start, int32_t S,
                     double *out, void *stream);
int nof_dbscan(const double *points, int32_t n, double eps, int32_t min_samples, const double *origin,
               const int32_t *dims, int32_t *labels, void *workspace, void *stream);

/* ------------------------------------------------------------------ group 5
 * Texture baking from the training images, the device
 * path of NerfRunner.mesh_texture_from_train_images (nerf_runner.py:1467-1541),
 * and vertex colours from the same images (SURVEY §8f row 2,
 * NerfRunner.mesh_vertex_color_from_train_images, nerf_runner.py:1431-1464).
 */

/* Depth + face-id z-buffer of a mesh seen by an OpenCV pinhole camera (the
 * reference's pyrender depth pass): zbuf [H*W] u64 = (f32 depth bits << 32 |
 * face), all ones where empty (this call fills it). Pixel centres at integer
 * (u, v); coverage edges inclusive, either winding; faces with a vertex at
 * z <= znear are skipped; depths beyond zfar are dropped. V [Nv,3] f32,
 * F [Fc,3] i64, ob_in_cam [4,4] f64 row-major, K [3,3] f64 row-major. */
int nof_raster_faces(const float *V, const int64_t *F, int64_t n_faces, const double *ob_in_cam, const double *K,
                     int32_t H, int32_t W, double znear, double zfar, uint64_t *zbuf, void *stream);

/* Per pixel of a z-buffer: where depth >= min_depth and mask [H*W] u8 is set,
 * the back-projected point (depth2xyzmap, Utils.py:219-231) moved to the
 * object frame by cam_in_ob [4,4] f64 and snapped to the closest point of the
 * rasterised face (trimesh.proximity.closest_point of the reference, on the
 * face the pixel sees): hit_locations [H*W,3] f32, hit_face_ids [H*W] i64
 * (-1 = no hit). */
int nof_texture_hits(const uint64_t *zbuf, int32_t H, int32_t W, const uint8_t *mask, float min_depth, const float *V,
                     const int64_t *F, const double *cam_in_ob, const double *K, float *hit_locations,
                     int64_t *hit_face_ids, void *stream);

/* nerf_runner.py:1524-1535 for one frame: texel = round-half-even(uvs[k])
 * flattened as y*(tex_w-1)+x (the reference's stride), the first hit k of
 * each texel adds colors[pix[k]] (f32 [*,3]) to tex [tex_h,tex_w,3] and 1 to
 * weight [tex_h,tex_w]. first: i32 [tex_h*(tex_w-1)+tex_w], all 0x7fffffff
 * on entry and on return. */
int nof_texture_accumulate(const float *uvs, const int32_t *pix, int64_t n_hits, const float *colors, int32_t tex_h,
                           int32_t tex_w, int32_t *first, float *tex, float *weight, void *stream);

/* One frame of NerfRunner.mesh_vertex_color_from_train_images (nerf_runner.py:
 * 1446-1458) without the reference's cKDTree. The candidates are the pixels of
 * a nof_raster_faces z-buffer that nof_texture_hits would take (a face, mask
 * set, depth >= min_depth), each at its back-projected point in the object
 * frame (no snap to the face). Per vertex V[j] (f32, widened to f64) the match
 * is the candidate with the smallest d2 = (dx*dx + dy*dy) + dz*dz in f64, ties
 * to the lowest pixel index; where sqrt(d2) <= radius its colour is added to
 * color_sum[j] and 1 to count[j] (plain adds by the vertex's own lane: no
 * atomics, deterministic). Only the screen window that bounds every candidate
 * within `radius` is searched, which needs ob_in_cam = inv(cam_in_ob), rigid,
 * and min_depth > 0. nearest / nearest_dist (either may be NULL) are written
 * for every vertex on every call: the accepted match's pixel index and
 * distance, -1 and +inf where there is none. n_vertices == 0 launches nothing. */
int nof_vertex_color_accumulate(const uint64_t *zbuf, int32_t H, int32_t W, const uint8_t *mask, float min_depth,
                                const float *colors,      /* [H*W,3] f32: the frame's image */
                                const double *cam_in_ob, const double *ob_in_cam, const double *K,
                                const float *V, int64_t n_vertices, double radius,
                                double *color_sum,        /* [Nv,3] f64, += */
                                int32_t *count,           /* [Nv] i32, += 1 */
                                int32_t *nearest,         /* [Nv] i32 or NULL: pixel index of the match, -1 = none */
                                double *nearest_dist,     /* [Nv] f64 or NULL: its distance, +inf = none */
                                void *stream);

/* Mesh render: depth, face id, colour and normal images of a triangle mesh at B poses in one call
 * (the reference's pyrender pass, offscreen_renderer.py: ModelRendererOffscreen). The z-buffer of
 * every pose is nof_raster_faces' (the same projection, cull, coverage and depth arithmetic and
 * the same 64-bit keys: ties in depth go to the lower face index), filled by two kernels: a lane
 * per (pose, face) rasterises the faces whose clamped bounding box holds at most small_max_pixels
 * pixels and lists the others, which a wave per listed face then rasterises 64 pixels at a
 * time. A third kernel shades every pixel; mesh_render.hip states its order of operations. */
enum { NOF_MESH_COLOUR_FLAT = 0, NOF_MESH_COLOUR_VERTEX = 1, NOF_MESH_COLOUR_TEXTURE = 2 };

typedef struct {
    const float *vertices;     /* device [n_vertices,3] f32, object frame */
    const int64_t *faces;      /* device [n_faces,3] i64, every corner in [0, n_vertices) (the caller's duty) */
    int64_t n_vertices;
    int64_t n_faces;           /* >= 0, and B n_faces < 2^31 */
    const uint8_t *colors;     /* device [n_vertices,3] u8 or NULL (needed by NOF_MESH_COLOUR_VERTEX) */
    const float *normals;      /* device [n_vertices,3] f32 or NULL: NULL shades with the face normal */
    const float *uv;           /* device [n_vertices,2] f32 or NULL (needed by NOF_MESH_COLOUR_TEXTURE) */
    const uint8_t *texture;    /* device [tex_h,tex_w,3] u8 or NULL, row 0 = top (as bake_texture stores it) */
    int32_t tex_h, tex_w;
    const double *ob_in_cam;   /* device [B,4,4] f64 row-major: object in the OpenCV camera */
    const double *K;           /* host [3,3] f64 row-major, read during the call */
    int32_t B, H, W;           /* B H W < 2^31 */
    double znear, zfar;        /* 0 < znear < zfar */
    int32_t colour_mode;       /* NOF_MESH_COLOUR_* */
    int32_t shade;             /* non-zero: the colour times |n . d|, d the unit pixel ray (a headlight) */
    uint8_t base_rgb[4];       /* NOF_MESH_COLOUR_FLAT's colour (3 used) */
    int32_t small_max_pixels;  /* >= 0: the largest bounding box the per-face lane rasterises itself */
    void *workspace;           /* device, nof_render_mesh_workspace_bytes(B, n_faces, H, W) bytes */
    float *depth;              /* device [B,H,W] f32: the z-buffer's depth, 0 on a miss */
    int32_t *face;             /* device [B,H,W] i32: the face seen, -1 on a miss */
    uint8_t *rgb;              /* device [B,H,W,3] u8, 0 on a miss */
    float *normal;             /* device [B,H,W,3] f32: unit, camera frame, towards the camera; 0 on a miss */
} nof_mesh_render_desc;

size_t nof_render_mesh_workspace_bytes(int32_t B, int64_t n_faces, int32_t H, int32_t W);

/* Two memsets and three launches on `stream`; nothing is read back. Every output pixel is written.
 * The result depends on the inputs alone (the z-buffer is built with atomicMin, which is
 * order-free): two calls give the same bits, and so does every small_max_pixels. The descriptor is
 * validated before the first HIP call: NOF_EINVAL with nof_last_error naming the field. */
int nof_render_mesh(const nof_mesh_render_desc *desc, void *stream);

/* ------------------------------------------------------------------ group 6
 * Mesh extraction on the device: the marching cubes of
 * NerfRunner.extract_mesh (nerf_runner.py:1349-1408, skimage there) and the
 * connected components of trimesh_split / largest_component (Utils.py:287-298,
 * bundlesdf.py:748-759). Both give what bundlesdf_amd/mesh.py's torch / scipy
 * code gives, bit for bit and in the same order.
 */

/* Shape check and launch geometry of the two calls below: volume [n0,n1,n2] with every n >= 2 and
 * n0 n1 n2 3 < 2^31 (NOF_EINVAL otherwise, nothing else is looked at); *n_blocks = blocks of 256
 * consecutive grid points (row-major, n2 fastest) = rows of block_counts / block_range / block_base. */
int nof_marching_cubes_blocks(int32_t n0, int32_t n1, int32_t n2, int64_t *n_blocks);

/* Counting pass. volume [n0,n1,n2] f32 contiguous; inside = value < level. tables [256,16] u8 from
 * bundlesdf_amd/mesh.py (device_tables): per case its triangle count, then 5 x 3 codes
 * corner | axis << 3 of the table edges (corner c = offset (c & 1, c >> 1 & 1, c >> 2 & 1) along
 * (n0, n1, n2), the case's bit c). Outputs: cells [points] u32, one word per grid point (its owned-edge
 * crossings, its cell's case and both block-local offsets: 4 bytes per grid point, the pass's only
 * volume-sized temporary); block_counts [n_blocks,2] i32 vertices and faces per block; block_range
 * [n_blocks,2] f32 smallest and largest value of the block. The shape is validated before anything
 * else, every argument before the launch. */
int nof_marching_cubes_count(const float *volume, int32_t n0, int32_t n1, int32_t n2, float level, const uint8_t *tables,
                             uint32_t *cells, int32_t *block_counts, float *block_range, void *stream);

/* Emit pass on the same volume / level / tables / cells. block_base [n_blocks,2] i64: the exclusive
 * prefix sums of block_counts' two columns; n_vertices, n_faces their totals. vertices [n_vertices,3]
 * f32 in index coordinates: the vertex of grid edge (q, axis a), q + clamp((level - v(q)) / (v(q + e_a)
 * - v(q)), 0, 1) e_a in f32 with an IEEE division, at position rank of linear(q) 3 + a among the crossed
 * edges. faces [n_faces,3] i32: cells in row-major order, a cell's triangles in table order, corners
 * [0, 2, 1] of the table row. Nothing is written past either total. */
int nof_marching_cubes_emit(const float *volume, int32_t n0, int32_t n1, int32_t n2, float level, const uint8_t *tables,
                            const uint32_t *cells, const int64_t *block_base, int64_t n_vertices, int64_t n_faces,
                            float *vertices, int32_t *faces, void *stream);

/* One sweep of connected-component labelling over a triangle list: faces [n_faces,3] i32 with
 * corners in [0, n_vertices) (other faces are skipped), labels [n_vertices] i32 with labels[v] <= v
 * (the caller starts from labels[v] = v). For every face the larger of its corners' roots are hooked
 * under the smallest (atomicMin), then every vertex is pointed at its root. *changed (device int,
 * cleared by the call) is set when a hook lowered a label; the caller repeats the call until it stays
 * 0 — every sweep that sets it lowers at least one label, so n_vertices + 1 sweeps bound the loop —
 * and then labels[v] is the smallest vertex index of v's component (a vertex in no face: itself). */
int nof_mesh_components(const int32_t *faces, int64_t n_faces, int64_t n_vertices, int32_t *labels, int32_t *changed,
                        void *stream);

/* Mesh smoothing: the tail of the reference's postprocess_mesh (run_custom.py:158-188,
 * trimesh.smoothing.filter_laplacian there). All of it is f64 in the stated operation order, without
 * contraction and without floating-point atomics, and no call waits for the host.
 *
 * One explicit (Jacobi) Laplacian step from v_in to v_out, both [V,3] f64 and distinct buffers. The
 * adjacency is CSR: row_start [V+1] i32, cols i32 (bundlesdf_amd/mesh.py vertex_adjacency: the distinct
 * neighbours of a vertex, ascending). For vertex i of degree d = row_start[i+1] - row_start[i] > 0, per
 * component: w = 1.0 / d, m = ((w v[j0] + w v[j1]) + w v[j2]) + ... over the row in stored order,
 * v_out[i] = v[i] + factor (m - v[i]). d == 0: v_out[i] = v[i] (trimesh's operator has a zero row there
 * and pulls the vertex towards the origin). A column outside [0, V) stands for vertex i itself. factor
 * must be finite; lamb for a Laplacian step, -nu for the odd steps of Taubin's filter. */
int nof_mesh_laplacian_step(const double *v_in, const int32_t *row_start, const int32_t *cols, int64_t V, double factor,
                            double *v_out, void *stream);

/* Signed volume of a triangle mesh, *volume_out (device f64) = (sum_f v0 . (v1 x v2)) / 6 with
 * c = (y1 z2 - z1 y2, z1 x2 - x1 z2, x1 y2 - y1 x2) and term = (x0 cx + y0 cy) + z0 cz. vertices [*,3]
 * f64, faces [F,3] i32 with every corner a valid vertex index (not checked: there is no vertex count).
 * A fixed thread-to-face assignment, a butterfly over the wave, the four waves added in order, one
 * partial per block in workspace (nof_mesh_volume_workspace_bytes(F) bytes, at most 1024 blocks), and
 * one block adds the partials in block order: the same bits on every run. F == 0 gives 0. */
size_t nof_mesh_volume_workspace_bytes(int64_t F);
int nof_mesh_volume(const double *vertices, const int32_t *faces, int64_t F, double *volume_out, void *workspace,
                    void *stream);

/* trimesh's volume constraint: every coordinate of vertices [V,3] f64 times s = cbrt(*vol_target /
 * *vol_now), about the origin. Both volumes are device f64. When the ratio is not a positive finite
 * number the vertices are left as they are and *flag (device i32, never cleared here) is set to 1. */
int nof_mesh_scale_to_volume(double *vertices, int64_t V, const double *vol_target, const double *vol_now, int32_t *flag,
                             void *stream);

/* Area-weighted vertex normals from the geometry: normals_out [V,3] f64. face_row_start [V+1] i32 /
 * face_ids i32 is the vertex -> face CSR (the faces of a vertex, each once, in ascending face index).
 * Per vertex s = 0, then s = s + (v1 - v0) x (v2 - v0) face by face in that order, with u = v1 - v0,
 * w = v2 - v0 and the cross product (uy wz - uz wy, uz wx - ux wz, ux wy - uy wx); len = sqrt((sx sx +
 * sy sy) + sz sz), normal = s / len (IEEE division), (0,0,0) when len is not > 0. A gather: no atomics.
 * A face with a corner outside [0, V) is skipped. */
int nof_mesh_vertex_normals(const double *vertices, const int32_t *faces, const int32_t *face_row_start,
                            const int32_t *face_ids, int64_t V, double *normals_out, void *stream);

/* ------------------------------------------------------------------ group 7
 * Pose and mesh evaluation (benchmark_ho3d.py:18-139 with Utils.py:82-103,
 * 268-273): the nearest-neighbour search behind ADD-S, the chamfer distance and
 * the point-to-point ICP before it (cKDTree and open3d there).
 */

/* Exact nearest neighbour of every query in a cloud of n points held in the grid
 * nof_point_grid_build made of it (cell_start, cell_points, cell_ids — required
 * here — and the same origin / dims / cell; at most 2^26 cells). queries [Q,3]
 * f64; xforms [B,4,4] f64 row-major or NULL (then B must be 1: the identity),
 * B <= 65535. For transform a the query is q = ((T[a][0] x + T[a][1] y) + T[a][2]
 * z) + T[a][3] per row, d2 = (dx dx + dy dy) + dz dz with dx = c_x - q_x, all in
 * f64 without contraction. index [B,Q] i32: the lowest input index among the
 * points of smallest d2; dist [B,Q] f64 = sqrt(d2). max_dist > 0: a query whose
 * dist is above it gets index -1 and dist +inf (max_dist <= 0: no limit).
 * Queries may lie anywhere, also outside the grid's box. Q == 0 or B == 0 returns
 * 0 at once; n == 0 with queries is NOF_EINVAL. */
int nof_nearest_points(const double *queries, int32_t Q, const double *xforms, int32_t B, const int32_t *cell_start,
                       const double *cell_points, const int32_t *cell_ids, int32_t n, const double *origin,
                       const int32_t *dims, double cell, double max_dist, int32_t *index, double *dist, void *stream);

/* The sums of one point-to-point registration step over the pairs (p'_i,
 * q_i = target[index[i]]) with 0 <= index[i] < m, where p' is source [n,3] f64
 * moved by xform [4,4] f64 row-major (device memory; NULL = identity) in the
 * operation order above: sums [17] f64 (device) = count, sum p' (3), sum q (3),
 * sum p' q^T (9, row-major: p' component first), sum dist[i]^2. Per-block partial
 * sums go to workspace (nof_nearest_workspace_bytes(n) bytes) and one block adds
 * them in block order: no floating-point atomics, the same bits on every run. */
size_t nof_nearest_workspace_bytes(int32_t n);
int nof_correspondence_moments(const double *source, int32_t n, const double *xform, const double *target, int32_t m,
                               const int32_t *index, const double *dist, double *sums, void *workspace, void *stream);

/* ------------------------------------------------------------------ group 8
 * Match filtering: multi-pair RANSAC over 3-D correspondences (the reference's
 * BundleTrack/src/cuda/cuda_ransac.cu behind SiftManager::runRansacMultiPairGPU:
 * which matches between two frames agree with one rigid motion).
 *
 * The correspondences of P frame pairs are concatenated: pair p owns the rows
 * pair_start[p] .. pair_start[p+1]-1 of pts_a / pts_b (n_p of them; the kernels
 * clamp both ends into [0, M] and never read outside it). The model maps A onto
 * B: b ~ R a + t. All arithmetic is f64 without contraction, in the order given
 * here, so the scores and flags of a pose can be reproduced bit for bit.
 *
 * Sampling. h(x) on uint32: x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15;
 *   x *= 0x846ca68b; x ^= x >> 16. Draw j in {0,1,2} of trial t of pair p is
 *   u = h((uint32)((p T + t) 3 + j) ^ h(seed)), the counter in wrapping uint32,
 *   and the row is (uint64(u) n_p) >> 32, local to the pair. A trial with two
 *   equal rows is dead (not redrawn); n_p < 3 makes every trial of the pair dead.
 * Hypothesis. The least-squares rigid fit of the three sampled pairs (Horn's unit
 *   quaternion: the eigenvector of the largest eigenvalue of the 4x4 matrix built
 *   from sum (a - mean a)(b - mean b)^T, by cyclic Jacobi rotations; R from the
 *   normalised quaternion, so it is a proper rotation for every sample, also a
 *   collinear or repeated one; t = mean b - R mean a). It is held to a float64
 *   SVD by tolerance, not bit for bit. A pose with a non-finite value is dead.
 * Gates. A trial is dead unless (tx tx + ty ty) + tz tz <= max_trans_sq[p] and
 *   (R00 + R11) + R22 >= min_trace[p] (= 1 + 2 cos(max_rot)); +inf / -inf switch
 *   a gate off. Dead trials score 0.
 * Inlier test of pose (R, t) and row i: q_k = ((R[k][0] ax + R[k][1] ay) +
 *   R[k][2] az) + t[k]; d2 = (dx dx + dy dy) + dz dz with dx = bx - qx; inlier iff
 *   d2 <= inlier_dist_sq and, with normals, (n'x mbx + n'y mby) + n'z mbz >=
 *   cos_normal where n'_k = (R[k][0] nx + R[k][1] ny) + R[k][2] nz (the normal of
 *   A rotated, not translated) and mb the normal of B.
 * Score. w_i = (int64) rint(conf_i 65536) with 0 <= conf_i <= 32767 (the caller's
 *   duty), 65536 without conf; a trial's score is the int64 sum of w_i over its
 *   inliers, accumulated with integer atomics: the same bits on every run.
 * Winner. Per pair the live trial of the highest score, the lowest trial among
 *   equals. No live trial with a score above 0: best_trial -1, score 0, the
 *   identity pose, no inliers.
 * Flags. inlier[i] is the inlier test of the pair's winning pose; n_inliers[p]
 *   their count. A pair with fewer than min_inliers inliers is cleared: flags 0,
 *   n_inliers 0 and sums 0, while best_trial, score and pose stay.
 * Sums. sums[p] has the layout of nof_correspondence_moments over the pair's
 *   inliers with the identity transform: count, sum a (3), sum b (3), sum a b^T
 *   (9, a's component first), sum d2 with d2 = (dx dx + dy dy) + dz dz, dx = bx -
 *   ax. One block per pair: thread r of 256 adds its rows r, r + 256, ... in
 *   order, a butterfly adds the lanes of a wave, the four waves are added in
 *   order. No floating-point atomics: the same bits on every run.
 */
typedef struct {
    const double *pts_a, *pts_b;          /* device [M,3] f64 */
    const double *normals_a, *normals_b;  /* device [M,3] f64, both or neither */
    const double *conf;                   /* device [M] f64 or NULL */
    const int32_t *pair_start;            /* device [P+1] i32 */
    const double *max_trans_sq;           /* device [P] f64 */
    const double *min_trace;              /* device [P] f64 */
    int64_t M;                            /* 0 <= M < 2^31 */
    int32_t P;                            /* 1 .. 65535 */
    int32_t n_trials;                     /* T: 1 .. 65536 */
    uint32_t seed;
    int32_t min_inliers;
    double inlier_dist_sq;                /* >= 0 */
    double cos_normal;                    /* used with normals only */
    void *workspace;                      /* device, at least nof_ransac_workspace_bytes(P, M, n_trials) */
    size_t workspace_bytes;               /* the size of workspace */
    int32_t *best_trial;                  /* device [P] i32 */
    int64_t *score;                       /* device [P] i64 */
    double *pose;                         /* device [P,16] f64, 4x4 row-major */
    int32_t *n_inliers;                   /* device [P] i32 */
    uint8_t *inlier;                      /* device [M] u8 */
    double *sums;                         /* device [P,17] f64 */
    /* debug outputs, NULL = not written */
    int32_t *trial_idx;                   /* device [P,T,3] i32: the rows drawn, local to the pair */
    double *trial_pose;                   /* device [P,T,12] f64: rows of [R | t]; zeros for a trial dead by its draws */
    uint8_t *trial_live;                  /* device [P,T] u8 */
    int64_t *trial_score;                 /* device [P,T] i64 */
} nof_ransac_desc;

/* Per-trial poses, live flags and scores: no [T x n] array exists anywhere. */
size_t nof_ransac_workspace_bytes(int32_t P, int64_t M, int32_t n_trials);

/* Four launches on `stream`; nothing is allocated or read back. The whole descriptor is validated
 * before the first HIP call: NOF_EINVAL with nof_last_error naming the field (P, n_trials and M
 * ranges, normals given on one side only, a NULL output, a negative or NaN inlier_dist_sq, a NULL
 * input or a workspace that is too small). M == 0 returns 0 at once without a launch: every pair is
 * empty and the outputs are left as the caller filled them (best_trial -1, the identity, zeros). */
int nof_ransac_pairs(const nof_ransac_desc *d, void *stream);

/* ------------------------------------------------------------------ group 9
 * Pose-graph optimisation over a window of N <= 128 frames (the reference's
 * CUDASolverBundling behind Bundler::optimizeGPU): n_outer Gauss-Newton steps over
 * camera-in-world poses, each one linearisation of a Huber-robust point-to-point
 * term over sparse matches (the layout of group 8: pair p owns rows pair_start[p] ..
 * pair_start[p+1]-1 of pts_a / pts_b, points of frame pair_frames[p] = (i, j) in
 * their cameras) plus a Huber-robust projective point-to-plane term between the
 * point / normal maps of every active pair of frames, n_inner steps of
 * Jacobi-preconditioned conjugate gradients on the explicit system, and the update
 * T_k <- Exp(delta_k) T_k. The definition, with the order of every operation, is
 * the header comment of bundlesdf_amd/csrc/pose_graph.hip. All arithmetic is f64
 * without contraction, every sum has a fixed order and no floating-point atomics
 * are used: the same bytes on every run. Iteration counts are fixed: no early
 * exit, nothing read back by the host.
 *
 * Either term may be absent (P == 0: no sparse term; points == NULL: no dense
 * term), not both. A frame with fixed[k] != 0 is a constant: its pose comes back
 * bit for bit, its rows and columns of A and g are zero. The caller makes sure at
 * least one frame is fixed (the gauge), that pair_start is monotone inside [0, M]
 * and that pair_frames names two different frames of 0 .. N-1; the kernels clamp
 * and skip rather than read outside an array.
 *
 * history [n_outer+1, 4] f64: sparse energy, dense energy, live sparse rows (weight
 * != 0), dense correspondences, at each linearisation and at the final poses. */
typedef struct {
    const double *poses;                  /* device [N,16] f64, 4x4 row-major camera-in-world */
    const uint8_t *fixed;                 /* device [N] u8 */
    int32_t N;                            /* 1 .. 128 */
    int32_t n_outer;                      /* 1 .. 1024 */
    int32_t n_inner;                      /* 0 .. 1024 */
    int32_t P;                            /* sparse pairs, 0 .. 65535 */
    int64_t M;                            /* sparse rows, 0 <= M < 2^31 */
    const int32_t *pair_frames;           /* device [P,2] i32 */
    const double *pts_a, *pts_b;          /* device [M,3] f64 */
    const int32_t *pair_start;            /* device [P+1] i32 */
    const double *weight;                 /* device [M] f64 or NULL (= 1); 0 drops the row */
    const float *points, *normals;        /* device [N,H,W,3] f32 camera-space maps, both or neither */
    int32_t H, W;                         /* H W < 2^24 */
    int32_t radius;                       /* window half-width of the correspondence search, 0 .. 32 */
    int32_t reserved;
    double fx, fy, cx, cy;                /* the maps' intrinsics */
    double robust_delta;                  /* Huber delta on the residual, > 0 */
    double w_sparse, w_dense;             /* >= 0 */
    double dist_thresh;                   /* > 0 */
    double normal_thresh;                 /* cosine */
    double depth_min, depth_max;          /* a point is valid if depth_min < z < depth_max */
    double min_trace;                     /* a pair is active iff trace(R_i^T R_j) > min_trace; -inf = always */
    void *workspace;                      /* device, at least nof_pose_graph_workspace_bytes(N, P, M, H, W) */
    size_t workspace_bytes;
    double *poses_out;                    /* device [N,16] f64 */
    double *history;                      /* device [n_outer+1,4] f64 */
    /* debug outputs, NULL = not written */
    double *iter_poses;                   /* device [n_outer+1,N,16] f64: the poses of every linearisation, then the final ones */
    double *dbg_A;                        /* device [n_outer,6N,6N] f64 */
    double *dbg_g;                        /* device [n_outer,6N] f64 */
    double *dbg_delta;                    /* device [n_outer,6N] f64 */
    int32_t *dense_index;                 /* device [n_outer,N,N,H W] i32, filled with -1 by the caller: entry (target i,
                                             source j, source pixel) = the chosen target pixel, written for active pairs */
} nof_pose_graph_desc;

/* Working poses, valid counts, per-(pair, chunk) partial sums, A, g and the history sums. H = W = 0
 * without a dense term. 0 for arguments out of range. */
size_t nof_pose_graph_workspace_bytes(int32_t N, int32_t P, int64_t M, int32_t H, int32_t W);

/* 1 + (n_outer + 1) x at most 4 launches on `stream`; nothing is allocated or read back. The whole
 * descriptor is validated before the first HIP call: NOF_EINVAL with nof_last_error naming the field
 * (N, n_outer, n_inner, P, M, neither term given, robust_delta, a NULL input or output, one map of two,
 * H, W, radius, dist_thresh, a weight below 0, a NaN threshold or intrinsic, workspace_bytes). */
int nof_pose_graph_optimize(const nof_pose_graph_desc *d, void *stream);

/* ------------------------------------------------------------------ group 10
 * Frame maps: from raw depth frames to what groups 8 and 9 start from (the
 * reference's Frame::processDepth, Frame::depthToCloudAndNormals and
 * Frame::invalidatePixelsByMask over BundleTrack/src/cuda/CUDAImageUtil.cu, with
 * SiftManager::makeCorrespondence and computeCovisibility), batched over N frames.
 *
 * Depth images are device [N,H,W] f32 in metres, row-major, pixel (u, v) = (column,
 * row); a non-finite depth is read as 0 everywhere. N is 1 .. 65535, H and W at
 * least 1, N H W < 2^31. The definition of every call, with the order of every
 * operation, is the header comment of bundlesdf_amd/csrc/frame_maps.hip: IEEE f64
 * without contraction from float32 inputs, outputs rounded once to float32,
 * thresholds taken as the doubles given here, no floating-point atomics, the same
 * bytes on every run. Every call launches on `stream`, allocates nothing, reads
 * nothing back, and validates its whole descriptor before the first HIP call:
 * NOF_EINVAL with nof_last_error naming the field.
 */

/* e = c unless the centre c fails c > depth_min and c <= zfar, or the share of bad
 * taps (x < depth_min or |x - c| > diff, taps outside the image not counted) of the
 * (2 radius + 1)^2 window reaches ratio; then e = 0. in and out are distinct. */
typedef struct {
    const float *in;                      /* device [N,H,W] f32 */
    float *out;                           /* device [N,H,W] f32 */
    int32_t N, H, W;
    int32_t radius;                       /* 0 .. 8 */
    double depth_min, zfar, diff, ratio;
} nof_frame_erode_desc;
int nof_frame_erode(const nof_frame_erode_desc *d, void *stream);

/* One pass of the reference's depth-aware Gaussian: the mean of the usable taps
 * (depth_min <= x <= zfar), then the weighted mean of the usable taps within band of
 * that mean, w = exp(-(dx^2 + dy^2) / two_sigma_d_sq - (c - x)^2 / two_sigma_r_sq);
 * 0 where no tap is usable or the weights sum to nothing. An invalid centre is
 * filled from its neighbours. in and out are distinct. */
typedef struct {
    const float *in;                      /* device [N,H,W] f32 */
    float *out;                           /* device [N,H,W] f32 */
    int32_t N, H, W;
    int32_t radius;                       /* 0 .. 8 */
    double depth_min, zfar;
    double two_sigma_d_sq, two_sigma_r_sq;  /* 2 sigma^2, formed by the caller, > 0 */
    double band;
} nof_frame_bilateral_desc;
int nof_frame_bilateral(const nof_frame_bilateral_desc *d, void *stream);

/* Camera-space points ((u - cx) z / fx, (v - cy) z / fy, z), normals by the
 * reference's central / one-sided differences, the grazing-angle filter (a pixel
 * with a normal is dropped if |n . P/|P|| < sin_edge), the mask, and the count of
 * the pixels left per frame. depth, points and normals are zero at every dropped
 * pixel, and every element is written. */
typedef struct {
    const float *depth_in;                /* device [N,H,W] f32 */
    const double *K;                      /* device [N,4] f64: fx, fy, cx, cy of each frame */
    const uint8_t *mask;                  /* device [N,H,W] u8, 0 drops the pixel; NULL = no mask */
    int32_t N, H, W;
    int32_t reserved;
    double depth_min;
    double z_diff;                        /* a neighbour takes part in a difference within this of the centre's z */
    double sin_edge;                      /* sin of the edge angle, formed by the caller */
    float *depth;                         /* device [N,H,W] f32, not depth_in */
    float *points, *normals;              /* device [N,H,W,3] f32 */
    int32_t *n_valid;                     /* device [N] i32, cleared by the call */
} nof_frame_geometry_desc;
int nof_frame_geometry(const nof_frame_geometry_desc *d, void *stream);

/* Pixel matches to 3-D matches, in the row layout of group 8: pair p owns rows
 * pair_start[p] .. pair_start[p+1]-1 and joins frames pair_frames[p] = (a, b). The
 * coordinates are rounded half away from zero, then bounds-checked; a row is valid
 * if both pixels exist, both z > depth_min and the optional gates pass (with poses,
 * camera-in-world: world distance <= max_dist, the unit world normals' dot product
 * >= cos_normal). Valid rows hold the maps' camera-space entries widened to f64,
 * invalid rows zeros; rows are not compacted. M == 0 returns 0 without a launch.
 * The caller makes sure pair_start is monotone from 0 to M. */
typedef struct {
    const float *points, *normals;        /* device [N,H,W,3] f32 */
    int32_t N, H, W;
    int32_t P;                            /* 1 .. 65535 */
    int64_t M;                            /* 0 <= M < 2^31 */
    const int32_t *pair_frames;           /* device [P,2] i32 */
    const int32_t *pair_start;            /* device [P+1] i32 */
    const double *uv_a, *uv_b;            /* device [M,2] f64: u (column), v (row) */
    const double *poses;                  /* device [N,16] f64 or NULL (no gates) */
    double depth_min;
    double max_dist;                      /* used with gate_dist */
    double cos_normal;                    /* used with gate_normal */
    int32_t gate_dist, gate_normal;       /* 0 = off */
    double *pts_a, *pts_b;                /* device [M,3] f64 */
    double *normals_a, *normals_b;        /* device [M,3] f64 */
    uint8_t *valid;                       /* device [M] u8 */
} nof_frame_lift_desc;
int nof_frame_lift_matches(const nof_frame_lift_desc *d, void *stream);

/* For each ordered pair q = (a, b): over every stride-th pixel of frame a from
 * (0, 0) with z >= depth_min and a non-zero normal, counts[q] = (visible, total),
 * visible where the unit direction from the moved point to the eye and the moved
 * unit normal have a dot product above cos_visible. T[q] = inv(pose_b) pose_a,
 * 4x4 row-major, formed by the caller. Q == 0 returns 0 without a launch. */
typedef struct {
    const float *points, *normals;        /* device [N,H,W,3] f32 */
    int32_t N, H, W;
    int32_t Q;                            /* 0 .. 65535 */
    const int32_t *pairs;                 /* device [Q,2] i32 */
    const double *T;                      /* device [Q,16] f64 */
    int32_t stride;                       /* >= 1 */
    int32_t reserved;
    double depth_min, cos_visible;
    int32_t *counts;                      /* device [Q,2] i32, cleared by the call */
} nof_frame_covis_desc;
int nof_frame_covisibility(const nof_frame_covis_desc *d, void *stream);

/* ------------------------------------------------------------------ group 11
 * Descriptor matching: the weight-free matching head of the reference's LoFTR
 * (BundleTrack/LoFTR/src/loftr/utils/coarse_matching.py: dual-softmax confidence,
 * threshold, border, mutual nearest neighbours), fused so that no [L,S] array is
 * ever written: what group 10's lift takes its pixel matches from.
 *
 * For P pairs, desc_a [P,L,C] and desc_b [P,S,C] are fp16 descriptors of the cells
 * of an h0 x w0 and an h1 x w1 grid (row-major, L = h0 w0, S = h1 w1).
 *   sim(i,j)  = (sum_k a_ik b_jk) * 1/(C temperature): fp16 products accumulated in
 *               f32 by the MFMA, one f32 scale applied to the sum; -inf where
 *               valid_a[i] or valid_b[j] is 0.
 *   conf(i,j) = exp(sim - rowmax_i) / rowsum_i * exp(sim - colmax_j) / colsum_j in
 *               f32 (row statistics over j, column statistics over i; a division is
 *               a product with the sum's f32 reciprocal). A row or column with no
 *               valid partner has max -inf, sum 0 and conf 0 everywhere.
 *   match     (i,j) iff conf(i,j) > thr, neither cell within border_rm cells of its
 *               grid's edge, j the lowest index attaining the maximum of row i and i
 *               the lowest index attaining the maximum of column j.
 * Every reduction runs in a fixed order and no floating-point atomic is used: the
 * same bytes on every run. csrc/match.hip's header comment is the full definition. */
typedef struct {
    const void *desc_a, *desc_b;          /* device [P,L,C] / [P,S,C] fp16, 16-byte aligned */
    const uint8_t *valid_a, *valid_b;     /* device [P,L] / [P,S] u8, both or neither */
    int32_t P;                            /* 1 .. 65535, P L and P S below 2^31 */
    int32_t L, S;                         /* h0 w0, h1 w1 */
    int32_t C;                            /* a multiple of 8 in 8 .. 512 */
    int32_t h0, w0, h1, w1;
    int32_t border_rm;                    /* >= 0 */
    int32_t reserved;
    float temperature;                    /* > 0 */
    float thr;                            /* in [0, 1) */
    void *workspace;                      /* device, at least nof_match_workspace_bytes(P, L, S) */
    size_t workspace_bytes;               /* the size of workspace */
    int32_t *j_of_i;                      /* device [P,L] i32: the match of row i, -1 for none */
    float *conf;                          /* device [P,L] f32: its confidence, 0 for none */
    int32_t *n_matches;                   /* device [P] i32 */
    /* debug outputs, NULL = kept in the workspace only */
    float *row_max, *row_sum;             /* device [P,L] f32 */
    float *col_max, *col_sum;             /* device [P,S] f32 */
} nof_match_desc;

/* Statistics and best partners per row and column: 7 arrays of P L or P S words, nothing of size L S. */
size_t nof_match_workspace_bytes(int32_t P, int32_t L, int32_t S);

/* Five launches on `stream` (statistics and best partner, each for rows and columns, then the
 * emit); nothing is allocated or read back. The whole descriptor is validated before the first HIP
 * call: NOF_EINVAL with nof_last_error naming the field. */
int nof_match_descriptors(const nof_match_desc *d, void *stream);

/* ------------------------------------------------------------------ group 12
 * Feature transformer: the reference's LocalFeatureTransformer (BundleTrack/LoFTR/
 * src/loftr/loftr_module/transformer.py, linear_attention.py), the stack of linear-
 * attention layers between a backbone and group 11's matching head, two fused kernels
 * and one fixed-order sum per layer application.
 *
 * One application x <- layer(x, source), x [L,C], source [S,C], 8 heads of D = C/8:
 *   Q = elu(x Wq^T) + 1, K = elu(source Wk^T) + 1, V = source Wv^T; Q *= x_mask,
 *   K *= source_mask, V *= source_mask (a mask byte of 0 takes the row out)
 *   KV_h = (1/S) sum_s K_h[s]^T V_h[s],  Ksum_h = sum_s K_h[s]
 *   msg_h[l] = (Q_h[l] KV_h) S / (Q_h[l] . Ksum_h + 1e-6)        S the full length
 *   m = LayerNorm1(msg Wm^T); m = LayerNorm2(relu([x | m] W1^T) W2^T); out = x + m
 *   (LayerNorm: eps 1e-5, biased variance, affine; no biases in the linear maps)
 * NOF_FT_SELF is a <- layer(a, a), b <- layer(b, b); NOF_FT_CROSS is a <- layer(a, b),
 * then b <- layer(b, a) with the updated a. feat_a and feat_b are float32 and are
 * updated in place. Every matrix product has fp16 operands and f32 accumulation; elu,
 * Z, the LayerNorm statistics and the residual add are f32, so a masked row and a
 * source with no unmasked row give finite values. Every sum runs in a fixed order and
 * no floating-point atomic is used: the same bytes on every run and for every batching.
 * csrc/feature_transformer.hip's header comment is the full definition.
 *
 * weights: n_layers blocks of 20 C C + 16 C bytes. A block holds Wq, Wk, Wv, Wm [C,C],
 * W1 [2C,2C] and W2 [C,2C] in fp16, each (out N, in K) matrix in fragment order
 * [N/32][K/16][64][8] with entry (nt, ks, lane, j) = W[32 nt + lane % 32][16 ks +
 * 8 (lane / 32) + j], then norm1.weight, norm1.bias, norm2.weight, norm2.bias [C] f32. */
#define NOF_FT_SELF 0
#define NOF_FT_CROSS 1
#define NOF_FT_MAX_LAYERS 16
typedef struct {
    float *feat_a, *feat_b;               /* device [P,L,C] / [P,S,C] f32, 16-byte aligned, read and overwritten */
    const uint8_t *mask_a, *mask_b;       /* device [P,L] / [P,S] u8 or NULL, each on its own */
    int32_t P;                            /* 1 .. 32767 (2 P problems in one launch) */
    int32_t L, S;                         /* >= 1 */
    int32_t C;                            /* 128 or 256 */
    int32_t n_layers;                     /* 1 .. NOF_FT_MAX_LAYERS */
    int32_t layer_kind[NOF_FT_MAX_LAYERS];/* NOF_FT_SELF or NOF_FT_CROSS, the first n_layers are read */
    int32_t reserved;
    const void *weights;                  /* device, 16-byte aligned, laid out as above */
    size_t weights_bytes;                 /* at least n_layers (20 C C + 16 C) */
    void *workspace;                      /* device, 16-byte aligned */
    size_t workspace_bytes;               /* at least the size the workspace function returns for (P, L, S, C) */
} nof_feature_transformer_desc;

/* Partial KV and Ksum of every block of 256 source rows, and their sums: 2 P problems; 0 for shapes
 * that are not supported. */
size_t nof_feature_transformer_workspace_bytes(int32_t P, int32_t L, int32_t S, int32_t C);

/* Three launches on `stream` per layer application (a self layer applies both sides in one set, a
 * cross layer takes two); nothing is allocated or read back. The whole descriptor is validated
 * before the first HIP call: NOF_EINVAL with nof_last_error naming the field. */
int nof_feature_transformer(const nof_feature_transformer_desc *d, void *stream);

/* ------------------------------------------------------------------ group 13
 * Fine-level match refinement: the reference's FinePreprocess (BundleTrack/LoFTR/src/
 * loftr/loftr_module/fine_preprocess.py) and FineMatching (utils/fine_matching.py),
 * the stages before and after its fine transformer, which is group 12 at C = 128
 * called on win_a / win_b in place between the two entry points.
 *
 * Match m has pair p = pair[m], cell i[m] of A's coarse grid h0 x w0 and cell j[m] of
 * B's h1 x w1; the fine maps are (stride h) x (stride w), channels-last fp16 with 128
 * channels, and pair p reads map frames_a[p] / frames_b[p] (map p without them).
 *   fine_window[r] = the fine feature at (stride (cell / w) + ky - 2, stride (cell % w)
 *                    + kx - 2), r = 5 ky + kx in 0..24, zeros outside the map
 *   ctx    = Wd coarse[p, cell] + b_down                        Wd [128,256]
 *   win[r] = Wm[:, :128] fine_window[r] + (Wm[:, 128:] ctx + b_merge)   Wm [128,256]
 *   sim[r] = win_a[12] . win_b[r] / sqrt(128), heat = softmax_r(sim)
 *   x = sum heat gx, y = sum heat gy, gx = -1 + kx / 2, gy = -1 + ky / 2
 *   std = sqrt(max(sum heat gx^2 - x^2, 1e-10)) + sqrt(max(sum heat gy^2 - y^2, 1e-10))
 * The three matrix products are MFMAs with fp16 operands and f32 accumulation; the
 * biases and ctx are added in f32; the correlation, the softmax and the moments are
 * f32. Every sum runs in a fixed order and no floating-point atomic is used: the same
 * bytes on every run and for every split of the matches into calls. A row whose pair,
 * cell or frame is out of range is written as zeros and nothing is read for it.
 * csrc/fine_match.hip's header comment is the full definition.
 *
 * weights: Wd [128,256], Wm[:, :128] and Wm[:, 128:] [128,128] in fp16, each in group
 * 12's fragment order, then b_down and b_merge [128] f32: 132096 bytes. */
typedef struct {
    const void *fine_a, *fine_b;          /* device [N_a,stride h0,stride w0,128] / [N_b,stride h1,stride w1,128] fp16 */
    const float *coarse_a, *coarse_b;     /* device [P,h0 w0,256] / [P,h1 w1,256] f32 */
    const int32_t *frames_a, *frames_b;   /* device [P] i32 or NULL, each on its own */
    const int32_t *pair, *i, *j;          /* device [M] i32 */
    int32_t M;                            /* 0 .. 2^24 */
    int32_t P;                            /* >= 1 */
    int32_t N_a, N_b;                     /* >= 1 */
    int32_t h0, w0, h1, w1;               /* >= 1, stride times each at most 32768 */
    int32_t stride;                       /* >= 1 */
    int32_t reserved;
    const void *weights;                  /* device, laid out as above */
    size_t weights_bytes;                 /* at least 132096 */
    float *context;                       /* device [2M,128] f32: ctx of side A's rows, then side B's */
    float *win_a, *win_b;                 /* device [M,25,128] f32 */
} nof_fine_windows_desc;

/* Two launches on `stream` (k_fine_context, k_fine_windows); nothing is allocated or read back.
 * fine_*, coarse_*, weights, context and win_* are 16-byte aligned. The whole descriptor is validated
 * before the first HIP call: NOF_EINVAL with nof_last_error naming the field. M == 0 returns NOF_OK
 * with no launch. */
int nof_fine_windows(const nof_fine_windows_desc *d, void *stream);

typedef struct {
    const float *win_a, *win_b;           /* device [M,25,128] f32, 16-byte aligned */
    const int32_t *pair, *i, *j;          /* device [M] i32 */
    int32_t M;                            /* 0 .. 2^24 */
    int32_t P;                            /* >= 1 */
    int32_t L, S;                         /* h0 w0, h1 w1 */
    float *expec;                         /* device [M,3] f32: x, y, std */
} nof_fine_expectation_desc;

/* One launch on `stream` (k_fine_expect); validated as above, M == 0 returns NOF_OK with no launch. */
int nof_fine_expectation(const nof_fine_expectation_desc *d, void *stream);

/* ------------------------------------------------------------------ group 14
 * LoFTR backbone: the reference's ResNetFPN_8_2 (BundleTrack/LoFTR/src/loftr/backbone/
 * resnet_fpn.py) in eval mode, initial_dim 128, block_dims [128, 196, 256]: a 7x7
 * stride-2 stem, three stages of two residual blocks at 1/2, 1/4 and 1/8 of the image,
 * and the FPN head. From N grey images (grey / 255) it gives the coarse tokens group 12
 * takes and the fine map group 13 takes. Every convolution is an implicit GEMM on
 * v_mfma_f32_32x32x16_f16 with fp16 operands (BatchNorm folded into the weights on the
 * host) and f32 accumulation; the bias, the residual, the bilinear upsample and the
 * activation are f32 and each activation is rounded once to fp16. Every sum runs in a
 * fixed order and no floating-point atomic is used: the same bytes on every run and for
 * every split of the images into calls. csrc/backbone.hip's header comment is the full
 * definition, with the layout of `weights` (bundlesdf_amd/backbone.py packs it). */
typedef struct {
    const float *images;                  /* device [N,H,W] f32 */
    int32_t N;                            /* >= 1 */
    int32_t H, W;                         /* multiples of 8, 8 .. 4096 */
    int32_t reserved;
    const void *weights;                  /* device, laid out as csrc/backbone.hip states */
    size_t weights_bytes;                 /* at least nof_backbone_weights_bytes() */
    const float *pe;                      /* device [H/8 W/8,256] f32 added to coarse, or NULL */
    float *coarse;                        /* device [N,H/8 W/8,256] f32 */
    void *fine;                           /* device [N,H/2,W/2,128] fp16, channels last */
    void *scratch;                        /* device */
    size_t scratch_bytes;                 /* at least nof_backbone_scratch_bytes(N, H, W) */
} nof_backbone_desc;

/* The activations of a call; 0 for shapes that are refused. */
size_t nof_backbone_scratch_bytes(int32_t N, int32_t H, int32_t W);
size_t nof_backbone_weights_bytes(void);

/* Twenty launches on `stream`; nothing is allocated or read back. images, weights, pe, coarse, fine and
 * scratch are 16-byte aligned. The whole descriptor is validated before the first HIP call: NOF_EINVAL
 * with nof_last_error naming the field. */
int nof_backbone(const nof_backbone_desc *d, void *stream);

/* ------------------------------------------------------------------ group 15
 * Pair crops: what the matcher is shown instead of whole frames (the reference's
 * Frame::updateRoi, BundleTrack/src/Frame.cpp, and the cv::warpPerspective calls of
 * processImagePair, BundleTrack/src/FeatureManager.cpp, over images zeroed outside the
 * mask). The per-pair transforms are formed on the host (bundlesdf_amd/pairs.py); the
 * warp takes their inverses. Pixel (u, v) = (column, row), images row-major. The
 * definition of both calls, with the order of every operation, is the header comment of
 * bundlesdf_amd/csrc/pair_crop.hip: IEEE f64 without contraction, outputs rounded once
 * to float32, integer atomics only, the same bytes on every run. Every call launches on
 * `stream`, allocates nothing, reads nothing back, and validates its whole descriptor
 * before the first HIP call: NOF_EINVAL with nof_last_error naming the field.
 */

/* roi[f] = (umin, umax, vmin, vmax), inclusive, over the pixels of frame f with mask > 0,
 * count[f] = their number; an empty mask gives (W, -1, H, -1) and 0. Both outputs are
 * initialised by the call. N is 0 .. 65535 (0 returns NOF_OK with no launch), H and W at
 * least 1, N H W < 2^31. */
typedef struct {
    const uint8_t *masks;                 /* device [N,H,W] u8 */
    int32_t N, H, W;
    int32_t reserved;
    int32_t *roi;                         /* device [N,4] i32 */
    int32_t *count;                       /* device [N] i32 */
} nof_mask_roi_desc;
int nof_mask_roi(const nof_mask_roi_desc *d, void *stream);

/* the element type and layout of nof_warp_images_desc.images */
#define NOF_WARP_GREY_U8 0                /* [N,H,W] u8, value / 255 */
#define NOF_WARP_GREY_F32 1               /* [N,H,W] f32, already in 0..1 */
#define NOF_WARP_RGB_U8 2                 /* [N,H,W,3] u8, (0.2989 R + 0.587 G) + 0.114 B per tap, / 255 */

/* Q square crops of side S, bilinear in f64: crop q reads frame frames[q] through inv[q],
 * the affine map from crop pixel (x, y) to source pixel. A tap outside the image, or
 * where masks is 0, reads 0. A crop whose frames[q] lies outside 0 .. N-1 is written as
 * zeros (cells too) and nothing is read for it. cells, when given, is 1 for each 8 x 8
 * cell of a crop with a pixel whose nearest source pixel lies inside the image and the
 * mask. S is a multiple of 8 in 8 .. 4096; Q >= 0 with Q ceil(S/32) < 2^31 (0 returns
 * NOF_OK with no launch); N is 1 .. 65535, N H W < 2^31. */
typedef struct {
    const void *images;                   /* device, as `format` says */
    const uint8_t *masks;                 /* device [N,H,W] u8 or NULL (no mask) */
    int32_t N, H, W;
    int32_t format;                       /* NOF_WARP_* */
    const int32_t *frames;                /* device [Q] i32 */
    const double *inv;                    /* device [Q,2,3] f64, row-major */
    int32_t Q, S;
    float *out;                           /* device [Q,S,S] f32 */
    uint8_t *cells;                       /* device [Q,S/8,S/8] u8 or NULL (not formed) */
} nof_warp_images_desc;
int nof_warp_images(const nof_warp_images_desc *d, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NOF_H */
