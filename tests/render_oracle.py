"""CPU oracle of the forward-only render (FusedStep.render_rays / nof_render_rays), composed of the
oracle's unchanged pieces — NS.pose_matrices, K.octree_ray_trace, K.sample_occupied,
NS.sample_rays_uniform(perturb=False), the grid forward (NS._GridFn), NS.nerf_small, NS.sh3 — plus a
restatement of raw2outputs (nerf_runner.py:1131-1168) and of render_images' depth rule (:602-610).
NS.trace_and_sample itself always perturbs, so its sampling part is restated here without draws."""
import numpy as np
import torch

from oracle import kernels as K
from oracle import nerf_step as NS


Z_TOL = dict(rtol=1e-6, atol=2e-6)   # the z tolerance of the forward parity tests (test_gpu_step.py:206)


def depth_rule(sdf, z, far_sc):
    """render_images :602-610 on float32 arrays [R,S]: signs = sdf[:,1:] * sdf[:,:-1]; rays whose signs
    are all > 0 read far_sc, the others z at the first negative sign (argmax of an all-false mask: 0)."""
    sdf, z = np.asarray(sdf, np.float32), np.asarray(z, np.float32)
    signs = sdf[:, 1:] * sdf[:, :-1]
    empty = (signs > 0).all(axis=-1)
    inds = np.argmax((signs < 0).astype(np.float32), axis=1)
    depth = np.take_along_axis(z, inds[:, None], axis=1)[:, 0].copy()
    depth[empty] = np.float32(far_sc)
    return depth, inds, empty


def trace_and_sample_unperturbed(batch, tf, occ, cfg, trunc, kmax=None):
    """render_rays :1043-1080 with perturb=False: z_vals [R, N + N_around] (octree samples, then the
    around-depth samples, unsorted)."""
    with torch.no_grad():
        sc = cfg["sc_factor"]
        R = batch.shape[0]
        N, Na = cfg["N_samples"], cfg["N_samples_around_depth"]
        rays_d = batch[:, 0:3]
        viewdirs = rays_d / rays_d.norm(dim=-1, keepdim=True)
        rays_o_w = tf[:, :3, 3]
        viewdirs_w = (tf[:, :3, :3] @ viewdirs[:, :, None])[:, :, 0]
        kb = 3 * occ.shape[0] if kmax is None else kmax
        dio, counts = K.octree_ray_trace(occ, rays_o_w.numpy(), viewdirs_w.numpy(), kb)
        dio = torch.from_numpy(dio[:, :max(1, int(counts.max()))].copy())
        depth = batch[:, 6]

        def occupied(dio_sub, vdirs, depths, n):
            z_in_out = dio_sub * torch.abs(vdirs[:, 2]).reshape(-1, 1, 1)
            if depths is not None:
                d = depths.reshape(-1, 1)
                valid = (d >= cfg["near"] * sc) & (d <= cfg["far"] * sc).expand(-1, z_in_out.shape[1])
                valid = valid & (z_in_out > 0).all(dim=-1)
                hi = (d.reshape(-1, 1, 1).expand(-1, z_in_out.shape[1], 2)[valid] + trunc)
                z_in_out[valid] = torch.clip(z_in_out[valid], min=torch.zeros_like(z_in_out[valid]), max=hi)
            total = NS._seqsum(z_in_out[:, :, 1] - z_in_out[:, :, 0])
            zc = NS.sample_rays_uniform(n, torch.zeros_like(total).reshape(-1, 1), total.reshape(-1, 1), None,
                                        perturb=False)
            zv, err = K.sample_occupied(z_in_out.numpy(), zc.numpy())
            assert err == 0, "sampler error"
            return torch.from_numpy(zv)

        z = occupied(dio, viewdirs, depth, N)
        vmask = (depth >= cfg["near"] * sc) & (depth <= cfg["far"] * sc)
        za = torch.zeros((R, Na))
        if vmask.any():
            za[vmask] = NS.sample_rays_uniform(Na, (depth[vmask] - trunc).reshape(-1, 1),
                                               (depth[vmask] + trunc * cfg["neg_trunc_ratio"]).reshape(-1, 1), None,
                                               perturb=False)
        if (~vmask).any():
            za[~vmask] = occupied(dio[~vmask], viewdirs[~vmask], None, Na)
        return torch.cat([z, za], -1)


def render(params, batch, c2w, occ, cfg, grid_meta, amp=False, step=0):
    """The render of batch [R,12] through the field `params` (as NS.train_step takes them): dict of
    z [R,S], valid [R,S], edge [R,S] (samples on a box face, see below), sdf [R,S], raw [R,S,4], rgb [R,3],
    depth [R] and the depth rule's (inds, empty)."""
    with torch.no_grad():
        sc = cfg["sc_factor"]
        P = {k: torch.as_tensor(v).detach().clone().float() for k, v in params.items()}
        batch, c2w = torch.as_tensor(batch).float(), torch.as_tensor(c2w).float()
        R = batch.shape[0]
        frame_ids = batch[:, 8].long()
        tf = NS.pose_matrices(P["pose"], frame_ids, cfg["max_trans"] * sc, cfg["max_rot"]) @ c2w[frame_ids]
        trunc = NS.truncation(cfg, step)
        z = trace_and_sample_unperturbed(batch, tf, occ, cfg, trunc)
        S = z.shape[1]
        rays_d = batch[:, 0:3]
        viewdirs = rays_d / rays_d.norm(dim=-1, keepdim=True)
        pts = rays_d[:, None, :] * z[:, :, None]
        tf_flat = tf[:, None].expand(-1, S, -1, -1).reshape(-1, 4, 4)
        x = (tf_flat[:, :3, :3] @ pts.reshape(-1, 3)[:, :, None] + tf_flat[:, :3, 3:])[:, :, 0]
        valid = (torch.abs(x) <= 1).all(dim=-1).view(R, S)
        # samples on a face of the box: unperturbed sampling puts a ray's first sample exactly where it
        # enters its first occupied voxel, which for many rays is the box face itself (|x| = 1 to the
        # last bit), so an implementation whose z differs by one ulp — inside Z_TOL — may decide
        # |x| <= 1 the other way there. `edge` marks the samples whose distance to a face is within
        # the position change Z_TOL allows, |d| (rtol z + atol), plus 1e-6 for the transform's rounding.
        margin = (torch.abs(x).max(dim=-1)[0] - 1).abs().view(R, S)
        edge = margin <= rays_d.norm(dim=-1, keepdim=True) * (Z_TOL["rtol"] * z.abs() + Z_TOL["atol"]) + 1e-6
        offsets, S_log, H = grid_meta
        emb_out = torch.zeros((R * S, (len(offsets) - 1) * P["embeddings"].shape[1]))
        vflat = valid.reshape(-1)
        if bool(vflat.any()):
            emb_out[vflat] = NS._GridFn.apply((x[vflat] + 1) / 2, P["embeddings"], offsets, S_log, H, amp, False)
        sh = NS.sh3((tf[:, :3, :3] @ viewdirs[:, :, None])[:, :, 0])
        parts = [emb_out]
        if "features" in P:
            parts.append(P["features"][frame_ids][:, None].expand(-1, S, -1).reshape(R * S, -1))
        parts.append(sh[:, None].expand(-1, S, -1).reshape(R * S, -1))
        raw = NS.nerf_small(torch.cat(parts, -1), P, amp).view(R, S, 4)
        # raw2outputs (:1131-1168)
        d = batch[:, 6].view(-1, 1)
        u = (d - z) / trunc
        w = torch.sigmoid(u * cfg["sdf_lambda"]) * torch.sigmoid(-u * cfg["sdf_lambda"])
        m = (z - d <= trunc * cfg["neg_trunc_ratio"]) & (z - d >= -trunc)
        w = torch.where((d > cfg["far"] * sc).expand(-1, S), torch.zeros_like(w), w * m)
        w = w / (w.sum(dim=-1, keepdim=True) + 1e-10)
        w = w * valid
        rgb = torch.sum(w[..., None] * torch.sigmoid(raw[..., :3]), -2)
        sdf = raw[..., 3].numpy()
        depth, inds, empty = depth_rule(sdf, z.numpy(), cfg["far"] * sc)
        return dict(z=z.numpy(), valid=valid.numpy(), edge=edge.numpy(), sdf=sdf, raw=raw.numpy(), rgb=rgb.numpy(), depth=depth,
                    inds=inds, empty=empty)
