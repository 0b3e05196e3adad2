"""CPU: the float64 pose oracle (tests/pose_oracle.py) checked on its own, before the device is
held to it in test_gpu_pose.py: in float32 it is oracle.nerf_step.pose_matrices bit for bit, its
float64 Jacobian agrees with central differences on both sides of the clamp, at data = 0 and
under a saturated tanh, frame 0 is the identity with a zero Jacobian whatever its row holds, and
the per-frame reduce drops ids outside [0,F). Also here, because it needs no device either: the
trainer refuses more frames than nof_pose_backward takes when it is built."""
import numpy as np
import pytest
import torch

from tests import pose_oracle as PO

MAX_TRANS, MAX_ROT = 0.02 * 6.6, 20.0


def test_fp32_oracle_is_pose_matrices_bit_for_bit():
    from oracle import nerf_step as NS
    rot = 35.0                    # the sweep reaches 0.55 rad: any direction fits under a 35 degree bound
    for F in (1, 2, 65):
        data, _, _ = PO.sweep_case(F, rot)
        want = NS.pose_matrices(data, torch.arange(F), MAX_TRANS, rot)
        got = PO.pose_matrices(data, MAX_TRANS, rot, torch.float32)
        assert got.dtype == torch.float32
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # the sweep puts frames on both sides of the clamp
    w = torch.tanh(data[1:, 3:].double()) * (rot / 180.0 * np.pi)
    below = int(((w * w).sum(-1) < PO.CLAMP).sum())
    assert 0.3 * (F - 1) < below < 0.7 * (F - 1)


def _fd_rows():
    rad = MAX_ROT / 180.0 * np.pi
    u = torch.tensor([0.3, -0.5, 0.81], dtype=torch.float64)
    u = u / u.norm()
    rows = [torch.full((6,), 1e3)]                                    # frame 0: ignored
    for norm in (3e-4, 0.009, 0.011, 0.2, 0.4):                       # both sides of |w| = 0.01
        rows.append(torch.cat([torch.tensor([0.4, -1.1, 0.2]), PO._rot_data(u * norm, MAX_ROT)]))
    rows.append(torch.zeros(6))                                       # data = 0
    rows.append(torch.full((6,), 30.0))                               # saturated tanh
    rows.append(torch.tensor([-30.0, 0.3, -30.0, 0.1, 30.0, -0.2]))
    assert abs(float(torch.tanh(rows[2][3:].double()).norm()) * rad - 0.009) < 1e-8
    return torch.stack(rows)


def test_fp64_jacobian_matches_central_differences():
    data = _fd_rows()
    F = data.shape[0]
    c2w = PO.random_rigid(F, torch.Generator().manual_seed(3))
    jac = PO.pose_jacobian(data, c2w, MAX_TRANS, MAX_ROT)
    assert jac.dtype == torch.float64 and jac.shape == (F, 12, 6)
    h = 1e-6
    d64 = data.double()
    fd = torch.zeros_like(jac)
    for p in range(6):
        e = torch.zeros(F, 6, dtype=torch.float64)
        e[:, p] = h
        hi = PO.pose_tf(d64 + e, c2w, MAX_TRANS, MAX_ROT)[:, :3, :].reshape(F, 12)
        lo = PO.pose_tf(d64 - e, c2w, MAX_TRANS, MAX_ROT)[:, :3, :].reshape(F, 12)
        fd[:, :, p] = (hi - lo) / (2 * h)
    # central differences: h^2 f''' / 6 ~ 1e-12 truncation, eps |tf| / h ~ 1e-9 cancellation (|tf| <~ 4)
    err = (jac - fd).abs().max(dim=1)[0].max(dim=1)[0]
    assert float(err.max()) < 1e-8, err
    assert float(jac[1:6].abs().amax(dim=(1, 2)).min()) > 1e-2        # and they are not trivially zero
    sat = data.abs() == 30.0
    assert (jac.permute(0, 2, 1)[sat] == 0).all()                     # 1 - tanh(30)^2 is exactly 0
    assert (jac[0] == 0).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_frame_zero_is_identity_with_zero_jacobian(dtype):
    g = torch.Generator().manual_seed(5)
    c2w = PO.random_rigid(3, g)
    for fill in (1e3, -1e3, 0.0, 0.3):
        data = torch.randn(3, 6, generator=g) * 0.5
        data[0] = fill
        T = PO.pose_matrices(data, MAX_TRANS, MAX_ROT, dtype)
        assert torch.equal(T[0], torch.eye(4, dtype=dtype))
        tf = PO.pose_tf(data, c2w, MAX_TRANS, MAX_ROT, dtype)
        assert torch.equal(tf[0], c2w[0].to(dtype))
        jac = PO.pose_jacobian(data, c2w, MAX_TRANS, MAX_ROT, dtype)
        assert jac.dtype == dtype and (jac[0] == 0).all() and torch.isfinite(jac).all()
        assert float(jac[1:].abs().max()) > 0


def test_frame_sums_drop_out_of_range_ids():
    g = torch.Generator().manual_seed(7)
    F, R = 5, 200
    rg = torch.randn(R, 12, generator=g)
    ids = torch.randint(0, F, (R,), generator=g)
    want = PO.frame_sums(rg, ids, F)
    assert want.dtype == torch.float64
    for f in range(F):
        assert torch.allclose(want[f], rg[ids == f].double().sum(0), rtol=0, atol=1e-12)
    bad = torch.tensor([-1, F, F + 5, -7, 2 ** 20])
    ids2 = torch.cat([ids, bad.repeat(8)])
    rg2 = torch.cat([rg, torch.randn(bad.numel() * 8, 12, generator=g) + 100.0])
    assert torch.equal(PO.frame_sums(rg2, ids2, F), want)
    assert torch.equal(PO.frame_sums(rg2[R:], ids2[R:], F), torch.zeros(F, 12, dtype=torch.float64))
    assert torch.equal(PO.frame_sums(rg[:0], ids[:0], F), torch.zeros(F, 12, dtype=torch.float64))
    # and pose_grad is the plain contraction
    jac = torch.randn(F, 12, 6, generator=g, dtype=torch.float64)
    gp = PO.pose_grad(want, jac)
    assert torch.allclose(gp[3], (want[3][:, None] * jac[3]).sum(0), rtol=0, atol=1e-12)


def test_fused_step_refuses_more_frames_than_the_pose_backward_takes():
    from bundlesdf_amd import fused
    assert fused.MAX_POSE_FRAMES == 1024
    c2w = torch.eye(4).repeat(fused.MAX_POSE_FRAMES + 1, 1, 1)
    with pytest.raises(ValueError, match="1024"):
        fused.FusedStep({}, torch.zeros(4, 12), c2w, None, None, None, None)
