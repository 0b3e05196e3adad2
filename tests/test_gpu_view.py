"""GPU: the free-camera surface render (nof_render_view / FusedStep.render_view / NerfRunner.render_view)
against its restatement in tests/view_oracle.py, in fp32 and amp, on a runner trained for 60 steps on the
synthetic scene (built as test_gpu_render.py builds its runner: a surface exists).

Parity: the oracle marches with sdf_fn = trainer.query_sdf and normal_fn = query_field's gradient, whose
bits the kernels reproduce, so hit and the coarse crossing index are compared for equality on every ray,
t and depth within 4 ulp, the normal within 1e-6, and the colour as tests/test_gpu_query.py compares
query_field's (fp32: rtol 1e-4, atol 1e-5; amp: within the oracle's own amp-vs-fp32 distance on the same
points). The worst entries go to profiles/r9/view_parity.json when NOF_WRITE_PARITY is set."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import query_oracle as QO
from tests import view_oracle as VO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [pytest.param(True, id="amp"), pytest.param(False, id="fp32")]
STATE = ("P", "M", "V", "Gbuf", "G16", "scale", "tracker", "found_inf", "adam_t", "step_dev", "loss_acc")
_PARITY = {}


def _runner(amp, frame_features=0):
    return _trained(bool(amp), int(frame_features))   # one cache entry per configuration


@functools.lru_cache(maxsize=None)
def _trained(amp, frame_features):
    from bundlesdf_amd import synthetic as SY
    from bundlesdf_amd.nerf_runner import NerfRunner
    seq = SY.make_sequence(3, seed=1)
    cfg = SY.default_cfg(sc_factor=seq["sc_factor"], translation=seq["translation"], n_step=60, N_rand=1024,
                         num_levels=16, amp=amp, frame_features=frame_features)
    nr = NerfRunner(cfg, seq["rgbs"], seq["depths"], seq["masks"], None, seq["poses"], seq["K"],
                    build_octree_pcd=seq["octree_pts"])
    nr.train()
    torch.cuda.synchronize()
    return nr, seq


def _small_K(nr, H, W, zoom=1.0):
    """The runner's camera scaled to an H x W image (zoom > 1 narrows it onto the object)."""
    K = np.asarray(nr.K, np.float64).copy()
    K[0, 0], K[1, 1] = K[0, 0] * W / nr.W * zoom, K[1, 1] * H / nr.H * zoom
    K[0, 2], K[1, 2] = (W - 1) / 2, (H - 1) / 2
    return K


def _field_fns(amp, frame_features=0, frame_id=0):
    return _field_fns_cached(bool(amp), int(frame_features), int(frame_id))


@functools.lru_cache(maxsize=None)
def _field_fns_cached(amp, frame_features, frame_id):
    nr, _ = _runner(amp, frame_features)
    tr = nr.trainer
    P = tr.split(tr.master_params().detach().cpu().clone())
    from oracle import nerf_step as NS
    meta = (tr.grid.offsets.cpu().numpy(), float(np.log2(tr.grid.per_level_scale)), int(tr.grid.base_resolution))
    Wd = {k: P[k] for k in NS.MLP_KEYS}
    ff = P["features"][frame_id].numpy() if frame_features else None

    def colour(mode_amp):
        return VO.colour_net(P["embeddings"], meta, Wd, amp=mode_amp, ff_row=ff)
    return (lambda p: tr.query_sdf(points=p), lambda p: tr.query_field(p, sdf=False, normals=True)["normals"], colour)


def _oracle(amp, c2w, K, H, W, frame_features=0, frame_id=0, colour_amp=None, **kw):
    nr, _ = _runner(amp, frame_features)
    tr = nr.trainer
    sdf_fn, normal_fn, colour = _field_fns(amp, frame_features, frame_id)
    kw.setdefault("step", 0.5 * nr.get_truncation())
    return VO.render(c2w, K, H, W, tr.occ.cpu().numpy(), tr.Kmax, sdf_fn, normal_fn,
                     colour(amp if colour_amp is None else colour_amp), **kw)


def _record(key, **figures):
    _PARITY[key] = {k: float(v) for k, v in figures.items()}
    print(key, _PARITY[key])
    if os.environ.get("NOF_WRITE_PARITY"):
        path = os.path.join(ROOT, os.environ["NOF_WRITE_PARITY"])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        old = json.load(open(path)) if os.path.exists(path) else {}
        old.update(_PARITY)
        with open(path, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)


def _check_parity(key, amp, got, ref, ref_other=None):
    """got: render_view(stats=True) flattened to numpy; ref: the oracle in the same mode; ref_other (amp):
    the oracle with the fp32 colour composition on the same points, for the allowance."""
    hit = ref["hit"].numpy()
    fig = dict(rays=hit.size, hits=int(hit.sum()))
    fig["t_ulp"] = int(VO.ulp_distance(got["t"], ref["t"].numpy()).max())
    fig["depth_ulp"] = int(VO.ulp_distance(got["depth"], ref["depth"].numpy()).max())
    fig["normal_abs"] = float(np.abs(got["normal"] - ref["normal"].numpy()).max())
    rgb_ref = ref["rgb"].numpy()
    fig["rgb_abs"] = float(np.abs(got["rgb"] - rgb_ref).max())
    if amp and hit.any():
        f32 = ref_other["rgb"].numpy()[hit]
        floor = float(np.linalg.norm(f32, axis=1).mean())
        fig["rgb_allowance"] = float(QO.normalised(rgb_ref[hit], f32, floor).max())
        fig["rgb_norm_err"] = float(QO.normalised(got["rgb"][hit], rgb_ref[hit], floor).max())
    _record(key, **fig)
    assert np.array_equal(got["hit"], hit)
    assert np.array_equal(got["index"], ref["index"].numpy())
    assert fig["t_ulp"] <= 4 and fig["depth_ulp"] <= 4, fig
    assert fig["normal_abs"] <= 1e-6, fig
    if amp:
        if hit.any():
            assert fig["rgb_norm_err"] <= fig["rgb_allowance"], fig
    else:
        np.testing.assert_allclose(got["rgb"], rgb_ref, rtol=1e-4, atol=1e-5)
    for k in ("t", "depth", "normal", "rgb"):
        assert not got[k][~hit].any(), k
    return fig


def _render(amp, c2w, K, H, W, frame_features=0, **kw):
    nr, _ = _runner(amp, frame_features)
    kw.setdefault("step", 0.5 * nr.get_truncation())
    r = nr.trainer.render_view(c2w, K, H, W, stats=True, **kw)
    return {k: v.reshape(-1, *v.shape[(1 if "pixels" in kw and kw["pixels"] is not None else 2):]).cpu().numpy()
            for k, v in r.items()}


def _parity_case(key, amp, c2w, K, H, W, **kw):
    got = _render(amp, c2w, K, H, W, **kw)
    ref = _oracle(amp, c2w, K, H, W, **kw)
    other = _oracle(amp, c2w, K, H, W, colour_amp=False, **kw) if amp else None
    return got, ref, _check_parity(key, amp, got, ref, other)


@pytest.mark.parametrize("amp", MODES)
def test_view_matches_oracle(cuda_device, amp):
    """1 x 1; 5 x 7 (a full 32-ray shading tile and a partial one); and steps that give the rays 33 or more
    samples, so that crossings fall in the first and in a later coarse tile."""
    nr, _ = _runner(amp)
    c2w = nr.poses[1]
    tag = "amp" if amp else "fp32"
    got, ref, _ = _parity_case(f"parity/{tag}/1x1", amp, c2w, _small_K(nr, 1, 1), 1, 1)
    assert ref["hit"].all()   # the centre pixel of a training view sees the object
    index = []
    step0 = 0.5 * nr.get_truncation()
    for div in (1, 2, 4):
        got, ref, fig = _parity_case(f"parity/{tag}/5x7/step_div{div}", amp, c2w, _small_K(nr, 5, 7, zoom=1.5), 5, 7,
                                     step=step0 / div)
        assert 0 < fig["hits"] < 35 or div > 1
        assert int(ref["ns"].max()) >= 33
        index.append(ref["index"][ref["hit"]].numpy())
    index = np.concatenate(index)
    assert (index < 32).any() and (index >= 32).any(), np.sort(index)


@pytest.mark.parametrize("amp", MODES)
def test_view_max_steps_widens_the_step(cuda_device, amp):
    nr, _ = _runner(amp)
    got, ref, fig = _parity_case(f"max_steps4/{'amp' if amp else 'fp32'}", amp, nr.poses[1], _small_K(nr, 5, 7, zoom=1.5),
                                 5, 7, max_steps=4)
    traced = ref["ns"] > 0
    assert traced.any() and int(ref["ns"].max()) <= 5
    assert (ref["step_eff"][traced] > 0.5 * nr.get_truncation()).all()
    assert (got["tiles"][traced.numpy()] == 1).all() and not got["tiles"][~traced.numpy()].any()


@pytest.mark.parametrize("amp", MODES)
def test_view_results_are_independent(cuda_device, amp):
    nr, _ = _runner(amp)
    c2w, K = nr.poses[1], _small_K(nr, 5, 7, zoom=1.5)
    one = _render(amp, c2w, K, 5, 7)
    assert one["hit"].any() and not one["hit"].all()
    for other in (_render(amp, c2w, K, 5, 7, chunk=32), _render(amp, c2w, K, 5, 7)):
        for k, v in one.items():
            assert np.array_equal(other[k], v), k
    pix = np.array([33, 2, 17, 34, 0, 16])
    sub = _render(amp, c2w, K, 5, 7, pixels=pix)
    uv = _render(amp, c2w, K, 5, 7, pixels=np.stack([pix % 7, pix // 7], 1))
    for k, v in one.items():
        assert sub[k].shape == (6,) + v.shape[1:] and np.array_equal(sub[k], v[pix]), k
        assert np.array_equal(uv[k], sub[k]), k
    full = nr.trainer.render_view(c2w, K, 5, 7)
    assert full["t"].shape == (5, 7) and full["normal"].shape == (5, 7, 3) and full["hit"].dtype == torch.bool
    assert set(full) == {"t", "depth", "normal", "rgb", "hit"}


@pytest.mark.parametrize("amp", MODES)
def test_view_misses_and_odd_cameras(cuda_device, amp):
    nr, _ = _runner(amp)
    tr = nr.trainer
    tag = "amp" if amp else "fp32"
    K = _small_K(nr, 5, 7, zoom=1.5)
    # turned away: the same position, looking the other way
    away = np.asarray(nr.poses[1], np.float64).copy()
    away[:3, :3] = away[:3, :3] @ np.diag([-1.0, 1.0, -1.0])
    got = _render(amp, away, K, 5, 7)
    assert not got["hit"].any()
    for k in ("t", "depth", "normal", "rgb"):
        assert not got[k].any(), k
    assert (got["index"] == -1).all()
    _parity_case(f"odd/{tag}/away", amp, away, K, 5, 7)
    # outside [-1,1]^3: the training pose pulled back along its viewing axis (GL cameras look down -z)
    out = np.asarray(nr.poses[1], np.float64).copy()
    out[:3, 3] += 2.5 * out[:3, 2]
    assert np.abs(out[:3, 3]).max() > 1
    _, ref, fig = _parity_case(f"odd/{tag}/outside", amp, out, _small_K(nr, 5, 7, zoom=6.0), 5, 7)
    assert fig["hits"] > 0
    # inside an occupied voxel, at the occupied voxel centre where the trained SDF is lowest (nudged off the
    # voxel faces): with a fine step sample 0 is already non-positive, the k = 0 rule
    occ = tr.occ.cpu().numpy()
    N = occ.shape[0]
    zyx = np.argwhere(occ > 0)
    ctr = (zyx[:, ::-1] + 0.5) * (2.0 / N) - 1
    sdf_c = tr.query_sdf(points=torch.from_numpy(ctr.astype(np.float32))).cpu().numpy()
    assert (sdf_c < 0).any()   # the trained object has an interior voxel centre
    inside = np.asarray(nr.poses[1], np.float64).copy()
    inside[:3, 3] = ctr[np.argmin(sdf_c)] + 0.123 / N   # off the voxel faces and centre planes
    _, ref, fig = _parity_case(f"odd/{tag}/inside", amp, inside, K, 5, 7, step=1e-3)
    assert (ref["index"][ref["hit"]] == 0).any()
    # a ray with more than Kmax intervals: this scene has none (the trainer's Kmax = 3 N is the most voxels a
    # DDA walk can cross); the most any ray of these views has is recorded
    many = int(ref["cnt"].max())
    _record(f"odd/{tag}/intervals", most_intervals=many, kmax=tr.Kmax)


@pytest.mark.parametrize("amp", MODES)
def test_view_frame_features_change_only_the_colour(cuda_device, amp):
    nr, _ = _runner(amp, 2)
    assert nr.trainer.n_ff == 2
    c2w, K = nr.poses[1], _small_K(nr, 5, 7, zoom=1.5)
    a = _render(amp, c2w, K, 5, 7, frame_features=2, frame_id=0)
    b = _render(amp, c2w, K, 5, 7, frame_features=2, frame_id=2)
    assert a["hit"].any()
    for k in ("t", "depth", "normal", "hit", "index"):
        assert np.array_equal(a[k], b[k]), k
    assert np.abs(a["rgb"] - b["rgb"]).max() > 1e-4
    for fid, got in ((0, a), (2, b)):
        ref = _oracle(amp, c2w, K, 5, 7, frame_features=2, frame_id=fid)
        other = _oracle(amp, c2w, K, 5, 7, frame_features=2, frame_id=fid, colour_amp=False) if amp else None
        _check_parity(f"ff/{'amp' if amp else 'fp32'}/frame{fid}", amp, got, ref, other)
    with pytest.raises(RuntimeError, match="frame_id"):
        nr.trainer.render_view(c2w, K, 5, 7, frame_id=3)


@pytest.mark.parametrize("amp", MODES)
def test_view_leaves_the_training_state_alone(cuda_device, amp):
    """The pattern of test_query_leaves_the_training_state_alone on a captured graph_step_ids: the replay
    after the render gives the bits a twin trainer's replay gives without one."""
    import bench
    from bundlesdf_amd.fused import FusedStep
    dev = cuda_device
    cfg, pool, frame_start, c2w, occ, _, _ = bench.build_rank_scene(0, 1, 4, dict(amp=amp, n_step=40), dev)

    def trainer():
        enc, net, pa = bench.make_models(cfg, len(frame_start) - 1, dev)
        return FusedStep(cfg, pool, torch.from_numpy(c2w), occ, enc, net, pa, amp=amp, frame_start=frame_start)
    plain, viewed = trainer(), trainer()
    ids = torch.arange(512, dtype=torch.int32, device=dev)
    K = np.array([[8.0, 0, 3.0], [0, 8.0, 2.0], [0, 0, 1]])
    outs = {}
    for name, fs in (("plain", plain), ("viewed", viewed)):
        fs.graph_step_ids(ids)
        torch.cuda.synchronize()
        if name == "viewed":
            snap = {k: getattr(fs, k).clone() for k in STATE if getattr(fs, k) is not None}
            graphs, step = fs._graphs, fs.global_step
            r = fs.render_view(c2w[1], K, 5, 7, step=0.02)
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(v.float()).all()) for v in r.values())
            for k, v in snap.items():
                assert torch.equal(getattr(fs, k), v), k
            assert fs._graphs is graphs and fs.global_step == step
        outs[name] = fs.graph_step_ids(ids)["loss_terms"].clone()
        torch.cuda.synchronize()
    # two trainers differ in low bits after a step (gradient atomics), so the twins are compared as
    # test_query_leaves_the_training_state_alone compares its eager and graph trainers
    torch.testing.assert_close(outs["viewed"][:6], outs["plain"][:6], rtol=2e-3, atol=1e-6)
    for name in ("P", "M", "V"):
        a, b = getattr(viewed, name), getattr(plain, name)
        assert float((a - b).norm() / b.norm().clamp_min(1e-30)) < 4e-3, name


def test_runner_render_view_and_script(cuda_device, tmp_path):
    nr, _ = _runner(True)
    r = nr.render_view(nr.poses[1], K=_small_K(nr, 12, 16), H=12, W=16)
    assert set(r) == {"t", "depth", "normal", "rgb", "hit"}
    assert r["t"].shape == r["depth"].shape == r["hit"].shape == (12, 16)
    assert r["normal"].shape == r["rgb"].shape == (12, 16, 3)
    assert r["t"].dtype == r["depth"].dtype == r["normal"].dtype == r["rgb"].dtype == np.float32
    assert r["hit"].dtype == np.bool_ and r["hit"].any()
    nrm = np.linalg.norm(r["normal"][r["hit"]], axis=1)
    assert np.all((np.abs(nrm - 1) < 1e-5) | (nrm == 0))
    m = nr.render_view(nr.poses[1], K=_small_K(nr, 12, 16), H=12, W=16, metres=True)
    sc = np.float32(nr.cfg["sc_factor"])
    assert np.array_equal(m["depth"], r["depth"] / sc) and np.array_equal(m["t"], r["t"] / sc)
    assert np.array_equal(m["rgb"], r["rgb"]) and np.array_equal(m["hit"], r["hit"])
    d = nr.render_view(nr.poses[1], pixels=[0, nr.W * (nr.H // 2) + nr.W // 2])   # K, H, W: the runner's own
    assert d["t"].shape == (2,) and d["hit"][1]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_view.py"), "--frames", "2", "--size",
                          "48x36", "--steps", "60", "--reps", "3", "--out", str(tmp_path / "tt"), "--json",
                          str(tmp_path / "rv.json")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    names = sorted(os.listdir(tmp_path / "tt"))
    assert names == sorted(f"view_{i:03d}_{k}.png" for i in range(2) for k in ("colour", "normal", "depth"))
    assert all(open(tmp_path / "tt" / n, "rb").read(8) == b"\x89PNG\r\n\x1a\n" for n in names)
    fig = json.load(open(tmp_path / "rv.json"))
    assert fig["size"] == [48, 36] and fig["rays"] == 48 * 36 and fig["render_view_ms"] > 0 and fig["render_rays_ms"] > 0
    assert 0 < fig["hit_share"] < 1 and fig["tiles_per_ray_mean"] > 0
