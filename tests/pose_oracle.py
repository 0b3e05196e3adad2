"""Plain restatement of the pose kernels (bundlesdf_amd/csrc/pose.hip) in torch, generic in the
dtype: float64 is the truth the device is held to, float32 is the reference's own precision and
serves only as the measuring stick for a tolerance.

  pose_matrices  PoseArray.get_matrices (nerf_helpers.py:127-154): tanh bound, pytorch3d
                 se3_exp_map with its 1e-4 clamp on |w|^2, transpose, frame 0 = identity. The op
                 sequence is that of oracle/nerf_step.py se3_exp_map / pose_matrices, so in
                 float32 the result is the same bits (tests/test_pose_oracle_cpu.py).
  pose_tf        tf = T @ c2w (nerf_runner.py:1050-1052)
  pose_jacobian  d tf[:3,:4] / d data [F,12,6], by autograd in the same dtype
  frame_sums     per-frame sums of ray_grad over the rays' frame ids; ids outside [0,F) dropped
  pose_grad      jac^T fg

Nothing here imports the package under test.
"""
import numpy as np
import torch

CLAMP = 1e-4      # se3_exp_map's eps on |w|^2


def _hat(v):
    x, y, z = v.unbind(-1)
    o = torch.zeros_like(x)
    return torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).view(*v.shape[:-1], 3, 3)


def se3_exp_map(log_transform, eps=CLAMP):
    """pytorch3d.transforms.se3_exp_map (published algorithm; row-vector convention)."""
    t, w = log_transform[..., :3], log_transform[..., 3:6]
    ang = torch.clamp((w * w).sum(-1), eps).sqrt()
    inv = 1.0 / ang
    fac1 = inv * ang.sin()
    fac2 = inv * inv * (1.0 - ang.cos())
    Kh = _hat(w)
    K2 = Kh @ Kh
    eye = torch.eye(3, dtype=log_transform.dtype)
    R = fac1[..., None, None] * Kh + fac2[..., None, None] * K2 + eye
    V = eye + Kh * ((1 - torch.cos(ang)) / ang ** 2)[..., None, None] + K2 * ((ang - torch.sin(ang)) / ang ** 3)[
        ..., None, None]
    T = (V @ t[..., None])[..., 0]
    out = torch.zeros((*log_transform.shape[:-1], 4, 4), dtype=log_transform.dtype)
    out[..., :3, :3] = R
    out[..., 3, :3] = T
    out[..., 3, 3] = 1.0
    return out


def pose_matrices(data, max_trans, max_rot_deg, dtype=torch.float64, eps=CLAMP):
    """T [F,4,4] of every frame (frame 0 the identity whatever data[0] holds)."""
    data = data.to(dtype)
    theta = torch.tanh(data)
    trans = theta[:, :3] * max_trans
    rot = theta[:, 3:6] * max_rot_deg / 180.0 * np.pi
    Ts_data = se3_exp_map(torch.cat((trans, rot), dim=-1), eps).permute(0, 2, 1)
    F = data.shape[0]
    ids = torch.arange(F)
    Ts = torch.eye(4, dtype=dtype).reshape(1, 4, 4).repeat(F, 1, 1)
    mask = ids != 0
    Ts[mask] = Ts_data[ids[mask]]
    return Ts


def random_rigid(F, gen):
    """c2w [F,4,4] f32: a random orthonormal block, a random translation, bottom row 0 0 0 1."""
    c2w = torch.eye(4).repeat(F, 1, 1)
    c2w[:, :3, :3] = torch.linalg.qr(torch.randn(F, 3, 3, generator=gen))[0]
    c2w[:, :3, 3] = torch.randn(F, 3, generator=gen)
    return c2w


def _rot_data(w, max_rot_deg):
    """The data entries whose bounded rotation is w (float64 [..,3]), rounded to float32."""
    return torch.atanh(w / (max_rot_deg / 180.0 * np.pi)).float()


EDGE_ULPS = (-4, -2, -1, 0, 1, 2, 4)     # |w| = 0.01 (1 + k 2^-23): |w|^2 within a few ulp of the clamp


def sweep_case(F, max_rot_deg, seed=0):
    """data [F,6] f32, c2w [F,4,4] f32 and the rows that need an exact check, for the forward tests.

    Frame 0 is filled with 1e3 (it must be ignored). The other frames sweep the rotation norm
    log-uniformly over 3e-4 .. 0.55 rad in random directions (the clamp edge is |w| = 0.01, so
    about half are clamped) with random translations. From F = 49 on, twelve of them are replaced
    by: an all-zero row, a row of +30, a row of -30, a row with every other entry at +-30
    (tanh saturates: those Jacobian columns are exactly 0), seven frames with |w| within a few
    ulp of the edge in a random direction and one on the x axis exactly at it.
    Returns (data, c2w, saturated) with saturated a bool [F,6] mask of the +-30 entries.
    """
    g = torch.Generator().manual_seed(1000 * seed + F)
    n = F - 1
    data = torch.zeros(F, 6)
    data[0] = 1e3
    if n > 0:
        t = torch.linspace(0, 1, n, dtype=torch.float64) if n > 1 else torch.tensor([0.5], dtype=torch.float64)
        norm = 3e-4 * (0.55 / 3e-4) ** t
        norm = norm[torch.randperm(n, generator=g)]       # no order along the frame index
        u = torch.randn(n, 3, generator=g, dtype=torch.float64)
        u = u / u.norm(dim=-1, keepdim=True)
        data[1:, 3:] = _rot_data(u * norm[:, None], max_rot_deg)
        data[1:, :3] = torch.randn(n, 3, generator=g) * 0.7
    if n >= 48:
        rows = []
        rows.append(torch.zeros(6))
        rows.append(torch.full((6,), 30.0))
        rows.append(torch.full((6,), -30.0))
        mixed = torch.randn(6, generator=g) * 0.3
        mixed[0::2] = torch.tensor([30.0, -30.0, 30.0])
        rows.append(mixed)
        for k in EDGE_ULPS:
            u = torch.randn(3, generator=g, dtype=torch.float64)
            w = u / u.norm() * (0.01 * (1.0 + k * 2.0 ** -23))
            rows.append(torch.cat([torch.randn(3, generator=g) * 0.7, _rot_data(w, max_rot_deg)]))
        rows.append(torch.cat([torch.randn(3, generator=g) * 0.7,
                               _rot_data(torch.tensor([0.01, 0.0, 0.0], dtype=torch.float64), max_rot_deg)]))
        stride = n // len(rows)
        for j, r in enumerate(rows):
            data[1 + j * stride] = r
    assert torch.isfinite(data).all(), "max_rot_deg must exceed 0.55 rad (31.6 deg) for the sweep to fit its bound"
    return data, random_rigid(F, g), data.abs() == 30.0


def pose_tf(data, c2w, max_trans, max_rot_deg, dtype=torch.float64, eps=CLAMP):
    """tf [F,4,4] = T(data) @ c2w."""
    return pose_matrices(data, max_trans, max_rot_deg, dtype, eps) @ c2w.to(dtype)


def pose_jacobian(data, c2w, max_trans, max_rot_deg, dtype=torch.float64, eps=CLAMP):
    """d tf[:3,:4] / d data as [F,12,6] (a frame's tf depends on its own row alone), by autograd."""
    d = data.detach().to(dtype).clone().requires_grad_(True)
    F = d.shape[0]
    rows = pose_tf(d, c2w, max_trans, max_rot_deg, dtype, eps)[:, :3, :].reshape(F, 12)
    jac = torch.zeros(F, 12, 6, dtype=dtype)
    for k in range(12):
        jac[:, k, :] = torch.autograd.grad(rows[:, k].sum(), d, retain_graph=True)[0]
    return jac


def frame_sums(ray_grad, frame_ids, F, dtype=torch.float64):
    """fg [F,12]: sum of ray_grad [R,12] over the rays of each frame; ids outside [0,F) are dropped."""
    ids = torch.as_tensor(frame_ids).to(torch.int64)
    keep = (ids >= 0) & (ids < F)
    fg = torch.zeros(F, 12, dtype=dtype)
    if int(keep.sum()):
        fg.index_add_(0, ids[keep], ray_grad.to(dtype)[keep])
    return fg


def pose_grad(fg, jac):
    """grad_pose [F,6] = sum_k fg[f,k] jac[f,k,:]."""
    return torch.einsum("fk,fkp->fp", fg, jac)
