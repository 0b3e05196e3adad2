"""GPU: nof_pose_forward / nof_pose_backward against torch autograd through the
oracle's PoseArray.get_matrices restatement (oracle/nerf_step.py pose_matrices,
nerf_helpers.py:127-154, pytorch3d se3_exp_map restated) and tf = T @ c2w
(nerf_runner.py:1050-1052): tf and the pose gradient within fp32 tolerance
(rtol 1e-5 / 1e-4), frame 0 identity with zero gradient, small-angle branch of
se3_exp_map (clamped norm) included."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_pose_forward_backward_matches_autograd(cuda_device):
    from bundlesdf_amd import _lib
    from bundlesdf_amd.nerf_helpers import PoseArray
    dev = cuda_device
    F, R = 7, 5000
    g = torch.Generator().manual_seed(0)
    pa = PoseArray(F, 0.02 * 6.6, 20.0)
    data = torch.randn(F, 6, generator=g) * 0.5
    data[2] = 1e-4 * torch.randn(6, generator=g)          # clamped-norm branch
    pa.data.data.copy_(data)
    c2w = torch.eye(4).repeat(F, 1, 1)
    c2w[:, :3, :3] = torch.linalg.qr(torch.randn(F, 3, 3, generator=g))[0]
    c2w[:, :3, 3] = torch.randn(F, 3, generator=g)
    # reference: autograd on CPU
    from oracle import nerf_step as NS
    T = NS.pose_matrices(pa.data, torch.arange(F), pa.max_trans, pa.max_rot)
    tf = T @ c2w
    frames = torch.randint(0, F, (R,), generator=g)
    ray_grad = torch.randn(R, 12, generator=g)
    fg = torch.zeros(F, 12).index_add_(0, frames, ray_grad)
    gp, = torch.autograd.grad(tf[:, :3, :].reshape(F, 12), pa.data, fg)
    # device
    L = _lib.lib()
    d_data = pa.data.detach().to(dev).contiguous()
    d_c2w = c2w.to(dev).contiguous()
    tf_out = torch.empty(F, 16, device=dev)
    jac = torch.empty(F, 12, 6, device=dev)
    _lib.check(L.nof_pose_forward(_lib.ptr(d_data), _lib.ptr(d_c2w), F, float(pa.max_trans),
                                  float(pa.max_rot / 180.0 * math.pi), _lib.ptr(tf_out), _lib.ptr(jac),
                                  _lib.stream_of(d_data)), "pose_forward")
    rays = torch.zeros(R, 12)
    rays[:, 8] = frames.float()
    d_rays, d_rg = rays.to(dev), ray_grad.to(dev)
    d_fg = torch.zeros(F, 12, device=dev)      # scratch: zero on entry, left zero
    d_gp = torch.zeros(F, 6, device=dev)
    _lib.check(L.nof_pose_backward(_lib.ptr(d_rg), _lib.ptr(d_rays), R, _lib.ptr(jac), F, _lib.ptr(d_fg),
                                   _lib.ptr(d_gp), _lib.stream_of(d_rg)), "pose_backward")
    torch.cuda.synchronize()
    np.testing.assert_allclose(tf_out.cpu().view(F, 4, 4).numpy(), tf.detach().numpy(), rtol=1e-5, atol=1e-6)
    assert float(d_fg.abs().max()) == 0.0          # the per-frame sums were consumed and cleared
    np.testing.assert_allclose(d_gp.cpu().numpy(), gp.numpy(), rtol=1e-4, atol=1e-4)
    assert (d_gp[0] == 0).all() and (jac[0] == 0).all()
    # PoseArray.get_matrices on the device runs the same kernel (c2w = identity)
    pa_d = PoseArray(F, pa.max_trans, pa.max_rot).to(dev)
    pa_d.data.data.copy_(pa.data.data)
    ids = torch.tensor([3, 0, 5, 5, 1])
    np.testing.assert_allclose(pa_d.get_matrices(ids).cpu().numpy(), T[ids].detach().numpy(), rtol=1e-5, atol=1e-6)
    # and the host (CPU) evaluation used by the hand-off tools agrees with both
    np.testing.assert_allclose(pa.get_matrices(ids).numpy(), T[ids].detach().numpy(), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------
# The three entry points of pose.hip against the float64 oracle (tests/pose_oracle.py), at many
# frames and at the edge shapes of each kernel. Tolerances come from the reference's own float32
# error on the same inputs (the oracle run in float32), never from the device's output.
import ctypes      # noqa: E402
import functools   # noqa: E402

from tests import pose_oracle as PO   # noqa: E402

MAX_TRANS, MAX_ROT = 0.02 * 6.6, 35.0       # 35 degrees: the sweep's 0.55 rad fits the bound in any direction
MAX_ROT_RAD = MAX_ROT / 180.0 * math.pi
FACTOR = 4.0          # device error <= FACTOR x the float32 oracle's error: another libm, another summation order
GUARD = 64            # guard elements on either side of every output buffer
SENT = 12345.0
EINVAL = 1            # NOF_EINVAL (include/nof.h)
U32 = 2.0 ** -24      # float32 unit roundoff


class _Guarded:
    """An output buffer of n elements filled with a sentinel, with GUARD sentinel elements on either side."""

    def __init__(self, n, dev, dtype=torch.float32, fill=SENT):
        self.n, self.fill = n, fill
        self.t = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=dev)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + GUARD * self.t.element_size())

    @property
    def body(self):
        return self.t[GUARD:GUARD + self.n]

    def guards_intact(self):
        return bool((self.t[:GUARD] == self.fill).all() and (self.t[GUARD + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.t == self.fill).all())


def _same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@functools.lru_cache(maxsize=None)
def _sweep_ref(F):
    """The forward case of F frames with its float64 truth and the float32 oracle's own worst errors."""
    data, c2w, sat = PO.sweep_case(F, MAX_ROT)
    tf64 = PO.pose_tf(data, c2w, MAX_TRANS, MAX_ROT)
    jac64 = PO.pose_jacobian(data, c2w, MAX_TRANS, MAX_ROT)
    tf32 = PO.pose_tf(data, c2w, MAX_TRANS, MAX_ROT, torch.float32)
    jac32 = PO.pose_jacobian(data, c2w, MAX_TRANS, MAX_ROT, torch.float32)
    e_tf = float((tf32.double() - tf64).abs().max())
    e_jac = float((jac32.double() - jac64).abs().max())
    return dict(data=data, c2w=c2w, sat=sat, tf64=tf64, jac64=jac64, jac32=jac32, e_tf=e_tf, e_jac=e_jac)


def _device_forward(dev, data, c2w):
    """nof_pose_forward into guarded, sentinel-filled buffers: (tf [F,16], jac [F,12,6]) on the device."""
    from bundlesdf_amd import _lib
    F = data.shape[0]
    d_data, d_c2w = data.to(dev).contiguous(), c2w.to(dev).contiguous()
    tf, jac = _Guarded(F * 16, dev), _Guarded(F * 72, dev)
    _lib.check(_lib.lib().nof_pose_forward(_lib.ptr(d_data), _lib.ptr(d_c2w), F, MAX_TRANS, MAX_ROT_RAD, tf.ptr,
                                           jac.ptr, _lib.stream_of(d_data)), "pose_forward")
    torch.cuda.synchronize()
    assert tf.guards_intact() and jac.guards_intact()
    return tf.body.view(F, 16), jac.body.view(F, 12, 6)


@pytest.mark.parametrize("F", [1, 2, 64, 65, 256, 257, 513, 1024])
def test_pose_forward_and_jacobian_against_float64(cuda_device, F):
    """tf and d tf / d data within 4x the float32 oracle's own worst error of the float64 oracle, over a
    log-uniform sweep of |w| across the clamp edge (pose_oracle.sweep_case), with frames a few ulp on either
    side of it, a zero row, saturated rows and frame 0 filled with 1e3; frame 0, the bottom rows and the
    saturated columns to the bit. F = 65 / 257 put frames in a second block of 64 lanes.

    Measured on an MI355X, device error / float32-oracle error as (tf, jac), held to 4 ("Pose
    kernels: what the tests hold them to"): F = 1 both exact (0 / 0); 2 (1.91, 1.03); 64 (1.00, 1.00);
    65 (1.09, 1.00); 256 (1.14, 1.00); 257 (1.35, 1.00); 513 (0.79, 1.00); 1024 (0.75, 1.00). The
    float32 oracle's errors themselves: tf 2e-8 (F = 2) .. 3.8e-7, jac 2e-6 (F = 2) .. 2.4e-5."""
    ref = _sweep_ref(F)
    tf, jac = _device_forward(cuda_device, ref["data"], ref["c2w"])
    tf, jac = tf.cpu(), jac.cpu()
    err_tf = float((tf.double().view(F, 4, 4) - ref["tf64"]).abs().max())
    err_jac = float((jac.double() - ref["jac64"]).abs().max())
    print(f"pose forward F={F}: tf {err_tf:.3e} / {ref['e_tf']:.3e} = {err_tf / max(ref['e_tf'], 1e-300):.2f}, "
          f"jac {err_jac:.3e} / {ref['e_jac']:.3e} = {err_jac / max(ref['e_jac'], 1e-300):.2f}")
    # exact
    c2w = ref["c2w"]
    assert (jac[0] == 0).all()
    assert _same_bits(tf[0], c2w[0].reshape(16))
    assert _same_bits(tf.view(F, 4, 4)[:, 3, :], c2w[:, 3, :])            # [0 0 0 1] @ c2w
    assert (jac.permute(0, 2, 1)[ref["sat"]] == 0).all()                   # 1 - tanh(+-30)^2 = 0
    assert torch.isfinite(tf).all() and torch.isfinite(jac).all()
    # within the reference's own precision
    assert err_tf <= FACTOR * ref["e_tf"], (err_tf, ref["e_tf"])
    assert err_jac <= FACTOR * ref["e_jac"], (err_jac, ref["e_jac"])


def test_pose_clamp_gradient_switches_exactly_at_the_edge(cuda_device):
    """torch.clamp(|w|^2, 1e-4) passes the gradient from |w|^2 == 1e-4 on and blocks it below. Across the
    edge the Jacobian jumps by only ~w^2/3 of itself (3e-5), well inside the float32 reference's
    cancellation error over the sweep above, so a wrong switch does not show there. Here it does: frames
    whose float32 |w|^2 is known to the bit (w on the x axis, a rotation bound of 64 = 2^6 so that
    w = 64 tanh(x) with tanh(x) = x to float32 rounding at x ~ 1.6e-4; float32(0.01)^2 rounds to
    float32(1e-4) exactly), c2w = identity, and the two entries d tf[1][2], d tf[2][1] / d data[3] =
    +-d(fac1 w)/dw, which carry no cancellation. The two float64 candidates (gradient passed / blocked:
    the oracle with eps just below / above the ladder) are 3e-5 apart; the device must sit on the right
    one for each of the ladder's k = -3..3 ulp, within 4x the float32 oracle's distance from its own
    (the float32 oracle only sets that scale: its bound goes through degrees, so its w is not the ladder's
    to the bit and it may switch a step early or late).
    Measured on an MI355X: candidates 2.1e-3 apart, float32 oracle 4.8e-6, device <= 8.6e-6 (ratio 1.8)."""
    from bundlesdf_amd import _lib
    dev = cuda_device
    m = np.float32(0.01)
    assert m * m == np.float32(1e-4)
    ladder = list(range(-3, 4))
    F = 1 + len(ladder)
    data = torch.zeros(F, 6)
    data[1:, :3] = torch.randn(F - 1, 3, generator=torch.Generator().manual_seed(29)) * 0.7
    for i, k in enumerate(ladder):
        w0 = m
        for _ in range(abs(k)):
            w0 = np.nextafter(w0, np.float32(1.0 if k > 0 else -1.0), dtype=np.float32)
        assert (w0 * w0 >= np.float32(1e-4)) == (k >= 0)
        data[1 + i, 3] = float(w0) / 64.0                       # exact: a power of two
    c2w = torch.eye(4).repeat(F, 1, 1)
    rot_deg = 64.0 * 180.0 / math.pi
    sel = lambda j: torch.stack([j[1:, 6, 3], -j[1:, 9, 3]], -1).double()      # noqa: E731  [ladder, 2]
    passed = sel(PO.pose_jacobian(data, c2w, MAX_TRANS, rot_deg, eps=PO.CLAMP * (1 - 1e-5)))
    blocked = sel(PO.pose_jacobian(data, c2w, MAX_TRANS, rot_deg, eps=PO.CLAMP * (1 + 1e-5)))
    gap = float((passed - blocked).abs().min())
    o32 = sel(PO.pose_jacobian(data, c2w, MAX_TRANS, rot_deg, torch.float32))
    e_ref = float(torch.minimum((o32 - passed).abs(), (o32 - blocked).abs()).max())
    assert gap > 10 * FACTOR * e_ref, (gap, e_ref)                              # no frame can satisfy both
    d_data, d_c2w = data.to(dev).contiguous(), c2w.to(dev).contiguous()
    tf, jac = _Guarded(F * 16, dev), _Guarded(F * 72, dev)
    _lib.check(_lib.lib().nof_pose_forward(_lib.ptr(d_data), _lib.ptr(d_c2w), F, MAX_TRANS, 64.0, tf.ptr, jac.ptr,
                                           _lib.stream_of(d_data)), "pose_forward")
    torch.cuda.synchronize()
    got = sel(jac.body.view(F, 12, 6).cpu())
    d_pass, d_block = (got - passed).abs().amax(-1), (got - blocked).abs().amax(-1)
    print(f"clamp ladder {ladder}: gap {gap:.3e}, float32 oracle {e_ref:.3e}, to 'passed' {d_pass.tolist()}, "
          f"to 'blocked' {d_block.tolist()}")
    for i, k in enumerate(ladder):
        near = d_pass[i] if k >= 0 else d_block[i]
        assert float(near) <= FACTOR * e_ref, (k, float(d_pass[i]), float(d_block[i]), e_ref)


# ------------------------------------------------------------------ the prologue equals its parts
N_STEP = 30
SCHED_STEPS = (0, 10, 11, 20, 21, N_STEP)


def _schedule(kind, n_step=N_STEP):
    from bundlesdf_amd import _lib
    return _lib.ScheduleDesc(lrate=0.01, lrate_pose=0.003, decay_rate=0.1, trunc=0.01, trunc_start=0.05,
                             sc_factor=6.6, trunc_decay=kind, n_step=n_step, seed_base=12345, batch_seed_base=777)


def _mlp_case(dev):
    from bundlesdf_amd import mlp_layout as ML
    assert ML.N_MLP == 9107
    idx, _, nfr = ML.pack_table()
    mlp = torch.randn(ML.N_MLP, generator=torch.Generator().manual_seed(11))
    n_frag = nfr * 64 * 8
    assert idx.size == n_frag + 5 * 64
    return mlp.to(dev), torch.from_numpy(idx).to(dev), n_frag, 5 * 64


@pytest.mark.parametrize("sched", [False, True], ids=["nosched", "sched"])
@pytest.mark.parametrize("amp", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("F", [1, 255, 256, 257, 513])
def test_step_prologue_equals_its_parts(cuda_device, F, amp, sched):
    """nof_step_prologue writes the bits of nof_pose_forward, nof_pack_mlp and (with a schedule)
    nof_step_schedule, and nothing beyond them: F = 256 / 257 / 513 move both boundaries of its block
    partition (one schedule block, ceil(F/256) pose blocks, the packing blocks after them)."""
    from bundlesdf_amd import _lib
    dev, L = cuda_device, _lib.lib()
    data, c2w, _ = PO.sweep_case(F, MAX_ROT)
    tf_ref, jac_ref = _device_forward(dev, data, c2w)
    mlp, idx, n_frag, n_bias = _mlp_case(dev)
    fdt, dcode = (torch.float16, 1) if amp else (torch.float32, 0)
    st = _lib.stream_of(mlp)
    frags_ref, bias_ref = _Guarded(n_frag, dev, fdt), _Guarded(n_bias, dev)
    _lib.check(L.nof_pack_mlp(_lib.ptr(mlp), _lib.ptr(idx), n_frag, n_bias, frags_ref.ptr, bias_ref.ptr, dcode, st),
               "pack_mlp")
    d_data, d_c2w = data.to(dev).contiguous(), c2w.to(dev).contiguous()
    tf, jac = _Guarded(F * 16, dev), _Guarded(F * 72, dev)
    frags, bias = _Guarded(n_frag, dev, fdt), _Guarded(n_bias, dev)
    outs = (tf, jac, frags, bias)

    def prologue(sd, step_ptr, sp_ptr):
        _lib.check(L.nof_step_prologue(sd, step_ptr, sp_ptr, _lib.ptr(d_data), _lib.ptr(d_c2w), F, MAX_TRANS,
                                       MAX_ROT_RAD, tf.ptr, jac.ptr, _lib.ptr(mlp), _lib.ptr(idx), n_frag, n_bias,
                                       frags.ptr, bias.ptr, dcode, st), "step_prologue")

    def check_parts():
        torch.cuda.synchronize()
        assert all(o.guards_intact() for o in outs)
        assert _same_bits(tf.body.view(F, 16), tf_ref) and _same_bits(jac.body.view(F, 12, 6), jac_ref)
        assert _same_bits(frags.body, frags_ref.body) and _same_bits(bias.body, bias_ref.body)

    SP = ctypes.sizeof(_lib.StepParams)
    if not sched:
        # no schedule: step and sp_out may be null ...
        prologue(None, None, None)
        check_parts()
        # ... and where they are given, they are neither read nor written
        for o in outs:
            o.t.fill_(o.fill)
        step = _Guarded(1, dev, torch.int32, fill=-77)
        sp = _Guarded(SP, dev, torch.uint8, fill=0xA5)
        prologue(None, step.ptr, sp.ptr)
        check_parts()
        assert step.untouched() and sp.untouched()
        return
    cases = [(kind, s) for kind in (0, 1, 2) for s in SCHED_STEPS]
    n = len(cases)
    start = torch.tensor([s for _, s in cases], dtype=torch.int32)
    step_a, step_b = _Guarded(n, dev, torch.int32, fill=-77), _Guarded(n, dev, torch.int32, fill=-77)
    step_a.body.copy_(start)
    step_b.body.copy_(start)
    sp_a, sp_b = _Guarded(n * SP, dev, torch.uint8, fill=0xA5), _Guarded(n * SP, dev, torch.uint8, fill=0xA5)
    for i, (kind, _) in enumerate(cases):
        sd = _schedule(kind)
        at = lambda g, sz: ctypes.c_void_p(g.ptr.value + i * sz)     # noqa: E731
        _lib.check(L.nof_step_schedule(ctypes.byref(sd), at(step_a, 4), at(sp_a, SP), st), "step_schedule")
        prologue(ctypes.byref(sd), at(step_b, 4), at(sp_b, SP))
    check_parts()
    assert step_a.guards_intact() and step_b.guards_intact() and sp_a.guards_intact() and sp_b.guards_intact()
    assert torch.equal(step_b.body.cpu(), start + 1) and torch.equal(step_a.body.cpu(), start + 1)
    blocks_a, blocks_b = sp_a.body.cpu().view(n, SP), sp_b.body.cpu().view(n, SP)
    for i, case in enumerate(cases):
        assert torch.equal(blocks_a[i], blocks_b[i]), case
        got = _lib.StepParams.from_buffer_copy(blocks_b[i].numpy().tobytes())
        assert got.step == case[1], case
    # the kinds differ where they should: the block is not a constant
    assert not torch.equal(blocks_b[1], blocks_b[1 + len(SCHED_STEPS)])


# ------------------------------------------------------------------ the reduce, exactly
REDUCE_SHAPES = [(1, 1), (1, 1024), (21, 7), (22, 300), (257, 7), (257, 1024), (10922, 300), (10923, 7),
                 (10923, 1024), (10925, 300), (20011, 1), (20011, 7), (20011, 1024)]
LAYOUTS = ["ascending", "one_frame", "descending", "shuffled", "out_of_range"]


def _reduce_case(R, F, layout):
    """ray_grad [R,12] (integers in [-8,8] x 2^-4, a third of them 0: any sum of them in any order is
    exact in float32) and the rays' frame ids under one of the layouts."""
    g = torch.Generator().manual_seed(R * 2048 + F)
    rg = torch.randint(-8, 9, (R, 12), generator=g).float() / 16.0
    rg[torch.rand(R, 12, generator=g) < 0.33] = 0.0
    ids = (torch.arange(R, dtype=torch.int64) * F) // R                 # ascending: the training layout
    asc = PO.frame_sums(rg, ids, F)
    if layout == "one_frame":
        ids = torch.full((R,), F // 2, dtype=torch.int64)
    elif layout in ("descending", "shuffled"):
        order = torch.arange(R - 1, -1, -1) if layout == "descending" else torch.randperm(R, generator=g)
        rg, ids = rg[order].contiguous(), ids[order]
    elif layout == "out_of_range":
        ids = ids.clone()
        bad = torch.tensor([-1, F, F + 5], dtype=torch.int64)
        ids[0::10] = bad[torch.arange(ids[0::10].numel()) % 3]
    want = PO.frame_sums(rg, ids, F)
    if layout in ("descending", "shuffled"):
        assert torch.equal(want, asc)            # the same rays in another order: the same sums
    w32 = want.float()
    assert torch.equal(w32.double(), want)       # exactly representable
    return rg, ids, w32


def _backward(dev, rg, ids, jac, fg, gp, F):
    from bundlesdf_amd import _lib
    R = rg.shape[0]
    rays = torch.zeros(R, 12)
    rays[:, 8] = ids.float()
    d_rg, d_rays = rg.to(dev).contiguous(), rays.to(dev).contiguous()
    st = _lib.stream_of(jac)
    return lambda: _lib.check(_lib.lib().nof_pose_backward(_lib.ptr(d_rg), _lib.ptr(d_rays), R, _lib.ptr(jac), F,
                                                           fg.ptr, gp.ptr, st), "pose_backward")


@functools.lru_cache(maxsize=None)
def _selectors(F):
    """jac[f][k][p] = (k == p) and (k == p + 6): grad_pose then receives the two halves of fg."""
    a, b = torch.zeros(F, 12, 6), torch.zeros(F, 12, 6)
    for p in range(6):
        a[:, p, p] = 1.0
        b[:, p + 6, p] = 1.0
    return a, b


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("R,F", REDUCE_SHAPES)
def test_pose_reduce_is_exact(cuda_device, R, F, layout):
    """k_pose_reduce + k_pose_grad with dyadic ray gradients and selector Jacobians: grad_pose must be
    start + the oracle's per-frame sums to the bit, fg all zero afterwards, and a second identical call
    must add the same again (the scratch was cleared, nothing else was). R = 10923 is the first batch
    whose grid is capped at 512 blocks; 10925 leaves blocks without rays; 21 / 22 straddle R*12 = 256."""
    dev = cuda_device
    rg, ids, want = _reduce_case(R, F, layout)
    g = torch.Generator().manual_seed(17)
    start = torch.randint(-64, 65, (F, 6), generator=g).float() / 8.0
    for half, sel in enumerate(_selectors(F)):
        jac = sel.to(dev)
        fg, gp = _Guarded(F * 12, dev, fill=0.0), _Guarded(F * 6, dev)
        fg.t[:GUARD] = SENT
        fg.t[GUARD + fg.n:] = SENT
        gp.body.copy_(start.reshape(-1))
        call = _backward(dev, rg, ids, jac, fg, gp, F)
        sums = want[:, 6 * half:6 * half + 6]
        for times in (1, 2):
            call()
            torch.cuda.synchronize()
            assert float(fg.body.abs().max()) == 0.0
            assert bool((fg.t[:GUARD] == SENT).all() and (fg.t[GUARD + fg.n:] == SENT).all())
            assert gp.guards_intact()
            assert _same_bits(gp.body.view(F, 6), start + times * sums), (half, times)


@pytest.mark.parametrize("F", [1, 1024])
def test_pose_backward_empty_batch(cuda_device, F):
    """R = 0 with null ray_grad / rays returns 0 and leaves grad_pose as it was."""
    from bundlesdf_amd import _lib
    dev = cuda_device
    jac = _selectors(F)[0].to(dev)
    start = torch.randint(-64, 65, (F, 6), generator=torch.Generator().manual_seed(19)).float() / 8.0
    fg, gp = _Guarded(F * 12, dev, fill=0.0), _Guarded(F * 6, dev)
    gp.body.copy_(start.reshape(-1))
    rc = _lib.lib().nof_pose_backward(None, None, 0, _lib.ptr(jac), F, fg.ptr, gp.ptr, _lib.stream_of(jac))
    torch.cuda.synchronize()
    assert rc == 0
    assert _same_bits(gp.body.view(F, 6), start) and gp.guards_intact() and fg.untouched()


# ------------------------------------------------------------------ the whole backward
@pytest.mark.parametrize("F", [257, 1024])
def test_pose_backward_against_float64(cuda_device, F):
    """nof_pose_forward's Jacobian through nof_pose_backward on 12000 rays in ascending frames against
    jac64^T (float64 sums). Per entry: 4x the float32 oracle's worst error of the same quantity, plus the
    summation-order term n_f u sum_r |g| |jac| of the frame's n_f rays (u = 2^-24, the worst case of any
    order of n_f float32 additions). Both parts come from the inputs."""
    dev = cuda_device
    ref = _sweep_ref(F)
    R = 12000
    g = torch.Generator().manual_seed(23)
    rg = torch.randn(R, 12, generator=g)
    ids = (torch.arange(R, dtype=torch.int64) * F) // R
    fg64 = PO.frame_sums(rg, ids, F)
    gp64 = PO.pose_grad(fg64, ref["jac64"])
    gp32 = PO.pose_grad(PO.frame_sums(rg, ids, F, torch.float32), ref["jac32"])
    e_ref = float((gp32.double() - gp64).abs().max())
    n_f = torch.bincount(ids, minlength=F).double()
    order = n_f[:, None] * U32 * PO.pose_grad(PO.frame_sums(rg.abs(), ids, F), ref["jac64"].abs())
    bound = FACTOR * e_ref + order
    _, jac = _device_forward(dev, ref["data"], ref["c2w"])
    fg, gp = _Guarded(F * 12, dev, fill=0.0), _Guarded(F * 6, dev, fill=0.0)
    _backward(dev, rg, ids, jac.contiguous(), fg, gp, F)()
    torch.cuda.synchronize()
    got = gp.body.view(F, 6).cpu().double()
    err = (got - gp64).abs()
    print(f"pose backward F={F}: worst err {float(err.max()):.3e}, float32 oracle {e_ref:.3e}, "
          f"worst err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, order term up to "
          f"{float(order.max()):.3e}")
    assert float(fg.body.abs().max()) == 0.0 and (got[0] == 0).all()
    assert float(gp64.abs().max()) > 1.0             # the case is not trivially small
    assert bool((err <= bound).all()), float((err - bound).max())


# ------------------------------------------------------------------ refused arguments
def test_pose_entry_points_refuse_bad_arguments(cuda_device):
    """Every bad call returns NOF_EINVAL before any launch: the error names the function, the
    sentinel-filled outputs are untouched, and the next valid call gives what it gave before."""
    from bundlesdf_amd import _lib
    dev, L = cuda_device, _lib.lib()
    F, R = 3, 40
    data, c2w, _ = PO.sweep_case(F, MAX_ROT)
    d_data, d_c2w = data.to(dev).contiguous(), c2w.to(dev).contiguous()
    mlp, idx, n_frag, n_bias = _mlp_case(dev)
    st = _lib.stream_of(mlp)
    tf, jac = _Guarded(F * 16, dev), _Guarded(F * 72, dev)
    frags, bias = _Guarded(n_frag, dev), _Guarded(n_bias, dev)
    step, sp = _Guarded(1, dev, torch.int32, fill=5), _Guarded(ctypes.sizeof(_lib.StepParams), dev, torch.uint8, 0xA5)
    rg, ids, _ = _reduce_case(R, F, "ascending")
    rays = torch.zeros(R, 12)
    rays[:, 8] = ids.float()
    d_rg, d_rays = rg.to(dev), rays.to(dev)
    big_jac = torch.zeros(1025, 12, 6, device=dev)
    fg, gp = _Guarded(1025 * 12, dev), _Guarded(1025 * 6, dev)
    outs = (tf, jac, frags, bias, step, sp, fg, gp)
    P = _lib.ptr

    def forward(F_=F, jac_=None):
        return L.nof_pose_forward(P(d_data), P(d_c2w), F_, MAX_TRANS, MAX_ROT_RAD, tf.ptr, jac.ptr if jac_ is None else jac_, st)

    def prologue(F_=F, jac_=None, dtype=0, sd=None):
        sdp = None if sd is None else ctypes.byref(sd)
        return L.nof_step_prologue(sdp, step.ptr if sd is not None else None, sp.ptr if sd is not None else None,
                                   P(d_data), P(d_c2w), F_, MAX_TRANS, MAX_ROT_RAD, tf.ptr, jac.ptr if jac_ is None else jac_, P(mlp),
                                   P(idx), n_frag, n_bias, frags.ptr, bias.ptr, dtype, st)

    def backward(F_=F, jac_=None):
        return L.nof_pose_backward(P(d_rg), P(d_rays), R, P(big_jac) if jac_ is None else jac_, F_, fg.ptr, gp.ptr, st)

    def valid():
        """One valid call of each entry point from fresh buffers: everything they write."""
        for o in outs:
            o.t.fill_(o.fill)
        fg.body.zero_()
        gp.body.zero_()
        assert forward() == 0
        a = (tf.body.clone(), jac.body.clone())
        assert prologue(sd=_schedule(1)) == 0
        assert backward() == 0
        torch.cuda.synchronize()
        assert all(o.guards_intact() for o in outs)
        return a + tuple(o.body.clone() for o in outs)

    first = valid()
    null = ctypes.c_void_p(0)
    refused = [("pose_forward", lambda: forward(F_=0)),
               ("step_prologue", lambda: prologue(F_=0)),
               ("pose_backward", lambda: backward(F_=0)),
               ("pose_backward", lambda: backward(F_=1025)),
               ("pose_forward", lambda: forward(jac_=null)),
               ("step_prologue", lambda: prologue(jac_=null)),
               ("pose_backward", lambda: backward(jac_=null)),
               ("step_prologue", lambda: prologue(dtype=7)),
               ("step_prologue", lambda: prologue(sd=_schedule(3))),
               ("step_prologue", lambda: prologue(sd=_schedule(1, n_step=0)))]
    for i, (name, call) in enumerate(refused):
        for o in outs:
            o.t.fill_(o.fill)
        rc = call()
        torch.cuda.synchronize()
        assert rc == EINVAL, (i, name, rc)
        assert name in L.nof_last_error().decode(), (i, name, L.nof_last_error())
        with pytest.raises(RuntimeError, match=name):
            _lib.check(rc, "caller")
        assert all(o.untouched() for o in outs), (i, name)
        again = valid()
        assert all(_same_bits(x, y) for x, y in zip(first, again)), (i, name)
    assert backward(F_=1024) == 0        # the limit itself is taken
    torch.cuda.synchronize()
