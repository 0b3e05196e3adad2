"""CPU: the render path's host side — nof_render_out's ctypes mirror, nof_render_rays' descriptor
validation (before any device work), the render oracle's depth rule on hand-made rows, and the
schedule of NerfRunner.train()'s periodic outputs with a stub trainer."""
import ctypes

import numpy as np
import pytest

from tests import render_oracle as RO


@pytest.fixture(scope="module")
def libnof():
    from bundlesdf_amd import build
    build.build()
    from bundlesdf_amd import _lib
    return _lib.lib()


def test_render_rays_refuses_bad_arguments_before_device_work(libnof):
    from bundlesdf_amd import _lib
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p).value

    def desc(**kw):
        D = _lib.FieldDesc()
        D.R, D.S, D.N_oct, D.N_dep, D.L, D.C, D.D, D.Kmax = 1, 64, 32, 32, 16, 2, 3, 8
        for k, v in kw.items():
            setattr(D, k, v)
        return D

    def call(D, O):
        rc = libnof.nof_render_rays(ctypes.byref(D), ctypes.byref(O), None)
        return rc, libnof.nof_last_error()

    rc, msg = call(desc(S=33), _lib.RenderOut(rgb=p, depth=p, workspace=p))
    assert rc == 1 and b"S=33" in msg
    rc, msg = call(desc(), _lib.RenderOut(depth=p, workspace=p))
    assert rc == 1 and b"rgb" in msg
    rc, msg = call(desc(), _lib.RenderOut(rgb=p, workspace=p))
    assert rc == 1 and b"depth" in msg
    rc, msg = call(desc(), _lib.RenderOut(rgb=p, depth=p))
    assert rc == 1 and b"rays" in msg            # the inputs are checked before the workspace ...
    rc, msg = call(desc(rays=p, tf=p, intervals=p, totals=p, table=p, levels=p, frags=p, bias=p),
                   _lib.RenderOut(rgb=p, depth=p))
    assert rc == 1 and b"workspace" in msg       # ... and every refusal comes before the first launch
    rc, msg = call(desc(L=17), _lib.RenderOut(rgb=p, depth=p, workspace=p))
    assert rc == 1 and b"L<=16" in msg
    # R == 0: success, nothing launched (no device here)
    assert libnof.nof_render_rays(ctypes.byref(desc(R=0)), ctypes.byref(_lib.RenderOut(rgb=p, depth=p)), None) == 0
    assert libnof.nof_render_workspace_bytes(96, 192) >= 96 * (128 + 6 * 48)
    assert libnof.nof_render_workspace_bytes(0, 192) == 0


def test_depth_rule_on_hand_made_rows():
    S, far = 192, 13.25
    z = np.arange(S, dtype=np.float32)[None].repeat(6, 0) + 0.5
    sdf = np.ones((6, S), np.float32)
    sdf[1, 32:] = -1                 # crossing at pair (31, 32)
    sdf[2, 128:] = -1                # crossing at pair (127, 128)
    sdf[3, 70] = 0                   # an exact zero, no negative product
    sdf[4] = 0                       # all zero
    sdf[5, 40:50] = -1               # two crossings: the first counts
    depth, inds, empty = RO.depth_rule(sdf, z, far)
    assert empty.tolist() == [True, False, False, False, False, False]
    assert inds.tolist()[1:] == [31, 127, 0, 0, 39]
    assert depth.tolist() == [np.float32(far), 31.5, 127.5, 0.5, 0.5, 39.5] and depth.dtype == np.float32


def test_validation_frame_choice():
    """train_loop :768-773."""
    from bundlesdf_amd.nerf_runner import validation_frames
    assert validation_frames([0]) == [0]
    assert validation_frames([3, 1, 0, 4, 2]) == [0, 1, 2, 3, 4]
    assert validation_frames(range(12)) == [0, 2, 4, 6, 8, 10, 11]


def _stub_runner(cfg):
    import torch
    from bundlesdf_amd.nerf_runner import NerfRunner

    class Trainer:
        time_kernels = True   # the eager branch of train(): step(ids=...)

        def __init__(self):
            self.calls = 0

        def step(self, ids=None):
            self.calls += 1
            return {"loss_terms": torch.zeros(8), "fs_rgb_loss": torch.zeros(())}

    class Loader:
        batch_size = 4

        def next_ids(self):
            return None

    nr = object.__new__(NerfRunner)
    nr.cfg, nr.N_iters, nr.global_step, nr._run = cfg, cfg["n_step"] + 1, 0, None
    nr.trainer, nr.data_loader = Trainer(), Loader()
    nr.fired = []
    for k in ("weights", "img", "print", "mesh", "pose"):
        setattr(nr, "_hook_" + k, lambda out, k=k: nr.fired.append((k, nr.global_step, nr.trainer.calls)))
    return nr


def test_hook_schedule_with_stub_trainer():
    nr = _stub_runner(dict(n_step=20, i_img=10, i_pose=10, i_weights=10, i_mesh=np.inf, i_print=999999))
    nr.train()
    # after the step that ran as g (g + 1 steps done), at g = 10 and 20 only, in train_loop's order
    assert nr.fired == [(k, g, g + 1) for g in (10, 20) for k in ("weights", "img", "pose")]
    assert nr.global_step == 21
    nr = _stub_runner(dict(n_step=20, i_img=np.inf, i_pose=np.inf, i_weights=np.inf, i_mesh=np.inf, i_print=np.inf))
    nr.train()
    assert nr.fired == []
    nr = _stub_runner(dict(n_step=20))   # missing keys: never
    nr.train()
    assert nr.fired == [] and nr.trainer.calls == 21
    nr = _stub_runner(dict(n_step=4, i_print=2, i_mesh=4))   # i_print has no g > 0 condition (:793)
    nr.train()
    assert nr.fired == [("print", 0, 1), ("print", 2, 3), ("print", 4, 5), ("mesh", 4, 5)]


def test_hook_periods():
    from bundlesdf_amd.nerf_runner import hook_periods, hooks_due
    assert hook_periods({}) == {} and hook_periods(dict(i_img=999999, i_mesh=np.inf, i_pose=0)) == {}
    p = hook_periods(dict(i_img=500, i_mesh=500.0, i_print=10))
    assert p == {"i_img": 500, "i_print": 10, "i_mesh": 500}
    assert hooks_due(p, 0) == ["i_print"] and hooks_due(p, 500) == ["i_img", "i_print", "i_mesh"]
    assert hooks_due(p, 250) == ["i_print"] and hooks_due(p, 7) == []
