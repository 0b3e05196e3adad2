"""CPU reference of the field point query (helper, not collected): SDF, d sdf / d point and colour,
composed only of what oracle/ exports — _GridFn on x01 of a leaf x, nerf_small, sh3 and torch autograd.

  sdf, normal: run_network_density(get_normals=True), nerf_runner.py:1306-1346 — the points are
    clipped to [-1, 1] and the CLIPPED tensor is the autograd leaf, grad_outputs = ones.
  colour: run_network as mesh_vertex_color_from_network calls it (:1411-1428, :1226-1303) — identity
    transform, view direction 0, one frame's features; a point with any |x| > 1 keeps a zero grid
    embedding (:1244-1265) and the nets still run; sigmoid of the three logits.

amp=True is the autocast composition: the fp16 table and dy_dx of grid_oracle.c's half mode, fp16
Linear results and input gradients (nerf_small(amp=True)), and the encoder's input-backward summed in
fp16 term by term in level order (_GridFn fp16_accum: kernel_input_backward in half)."""
import numpy as np
import torch

from oracle import nerf_step as NS


def field_query(pts, emb, offsets, S_log, H, W, amp=False, ff_row=None, mlp_double=False):
    """pts [n,3]; emb [T,2] float tensor; (offsets, S_log, H) the grid meta of oracle.nerf_step; W the
    MLP state dict (float tensors); ff_row: the frame's feature row or None. mlp_double (fp32 only):
    the MLP part in float64 on the float32 encoder output (the encoder stays the C oracle's fp32).
    Returns float32 / float64 tensors: sdf [n], normal [n,3], rgb [n,3], pre1 [n,64] (the layer-1
    pre-activations, so tests can set kink points aside)."""
    assert not (amp and mlp_double)
    pts = torch.as_tensor(np.asarray(pts), dtype=torch.float32)
    n = pts.shape[0]
    dt = torch.float64 if mlp_double else torch.float32
    Wd = {k: v.detach().to(dt) for k, v in W.items()}
    n_ff = 0 if ff_row is None else len(ff_row)
    views = torch.zeros(n, n_ff + 9, dtype=dt)
    if n_ff:
        views[:, :n_ff] = torch.as_tensor(np.asarray(ff_row), dtype=dt)
    views[:, n_ff:] = NS.sh3(torch.zeros(n, 3, dtype=dt))

    x = torch.clip(pts, -1, 1).clone().requires_grad_(True)
    x01 = (x + 1) / 2
    feat = NS._GridFn.apply(x01, emb.detach().float(), offsets, S_log, H, amp, amp)
    acts = {}
    out = NS.nerf_small(torch.cat([feat.to(dt), views], -1), Wd, amp, acts)
    sdf = out[:, 3]
    (normal,) = torch.autograd.grad(sdf, x, grad_outputs=torch.ones_like(sdf))
    pre1 = acts["sigma_net.0"][1].detach()

    with torch.no_grad():
        inside = (pts.abs() <= 1).all(-1)
        e = torch.where(inside[:, None], feat.detach().to(dt), torch.zeros((), dtype=dt))
        rgb = torch.sigmoid(NS.nerf_small(torch.cat([e, views], -1), Wd, amp)[:, :3])
    return dict(sdf=sdf.detach(), normal=normal.detach(), rgb=rgb, pre1=pre1)


# ---- the GPU tests' fields and point sets (built once per configuration, shared, never modified)
CONFIGS = {
    # tests/golden/train_step.npz as test_query_sdf_matches_oracle uses it: 4 levels (16 .. 32), every one
    # hashed (17^3 > 2^12 rows), L < 16 (the lanes of the absent levels), embeddings x 300
    "golden": dict(),
    # 8 levels 4 .. 128 in 2^12 rows: the lower four dense, the upper four hashed
    "mixed": dict(num_levels=8, base_res=4, finest_res=128, log2_hashmap_size=12),
    # the same with two frame features
    "mixed_ff": dict(num_levels=8, base_res=4, finest_res=128, log2_hashmap_size=12, frame_features=2),
}


def point_set(n, scale0, seed=0):
    """n points: inside the box, exactly on +-1, outside it (up to +-1.1) and on cell corners of the
    coarsest level (x01 scale0 + 0.5 an integer), interleaved so every prefix holds all four kinds."""
    rng = np.random.default_rng(seed)
    m = (n + 3) // 4
    inside = rng.uniform(-1, 1, (m, 3))
    face = rng.uniform(-1, 1, (m, 3))
    ax = rng.integers(0, 3, m)
    face[np.arange(m), ax] = rng.choice([-1.0, 1.0], m)
    face[::5] = np.sign(face[::5])                      # some on edges / vertices of the box
    out = rng.uniform(-1, 1, (m, 3))
    out[np.arange(m), ax] = rng.choice([-1.0, 1.0], m) * rng.uniform(1.0, 1.1, m)
    out[::3] = rng.uniform(-1.1, 1.1, (len(out[::3]), 3))
    k = rng.integers(1, int(scale0), (m, 3))
    corner = 2 * (k - 0.5) / scale0 - 1
    corner[1::2, 1:] = rng.uniform(-1, 1, (len(corner[1::2]), 2))   # on a cell face only
    pts = np.stack([inside, face, out, corner], 1).reshape(-1, 3)[:n]
    return pts.astype(np.float32)


def make_case(name, n=3000):
    """Parameters, points and the CPU references of one configuration (CPU only)."""
    import json
    import os
    from bundlesdf_amd.grid import level_layout
    from bundlesdf_amd.nerf_helpers import NeRFSmall
    from oracle import kernels as K
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "train_step.npz"))
    cfg = dict(json.loads(str(g["cfg_json"])), **CONFIGS[name])
    L, n_ff = cfg["num_levels"], cfg.get("frame_features", 0)
    pls, offsets = level_layout(3, L, 2, cfg["base_res"], cfg["log2_hashmap_size"], cfg["finest_res"])
    S_log = float(np.log2(pls))
    rng = np.random.default_rng(7)
    if name == "golden":
        emb = torch.from_numpy(g["emb0"]) * 300
        W = {k: torch.from_numpy(g["w0_" + k]) for k in NS.MLP_KEYS}
    else:
        emb = torch.from_numpy(rng.uniform(-0.03, 0.03, (int(offsets[-1]), 2)).astype(np.float32))
        torch.manual_seed(7)
        net = NeRFSmall(2, 64, 15, 3, 64, input_ch=2 * L, input_ch_views=9 + n_ff)
        W = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ff = torch.from_numpy(rng.normal(0, 1, (3, n_ff)).astype(np.float32)) if n_ff else None
    scales, _ = K.level_params(L, S_log, cfg["base_res"])
    pts = point_set(n, float(scales[0]))
    meta = (offsets, S_log, cfg["base_res"])
    case = dict(name=name, cfg=cfg, emb=emb, W=W, ff=ff, pts=pts, meta=meta, golden=g)
    for fid in range(2 if n_ff else 1):
        row = None if ff is None else ff[fid].numpy()
        case[("fp32", fid)] = field_query(pts, emb, *meta, W, ff_row=row)
        case[("amp", fid)] = field_query(pts, emb, *meta, W, amp=True, ff_row=row)
    case["f64"] = field_query(pts, emb, *meta, W, mlp_double=True, ff_row=None if ff is None else ff[0].numpy())
    return case


def normalised(a, ref, floor):
    """Per-point |a - ref|_2 / (|ref|_2 + floor)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(a - ref, axis=1) / (np.linalg.norm(ref, axis=1) + floor)


def kink_points(case):
    """amp: points with a layer-1 pre-activation of the amp oracle within the oracle's own amp-vs-fp32
    pre-activation difference (its maximum over the set: one threshold per configuration) of zero —
    an implementation rounding differently may take the other side of that ReLU there."""
    pa, pf = case[("amp", 0)]["pre1"].numpy(), case[("fp32", 0)]["pre1"].numpy()
    delta = float(np.abs(pa - pf).max())
    return (np.abs(pa) <= delta).any(1), delta
