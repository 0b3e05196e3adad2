"""GPU: the field point query (nof_query_field / FusedStep.query_field) against the CPU oracle of
tests/query_oracle.py — SDF bit-identical to query_sdf, the analytic normal in fp32 and amp, the clip
semantics, the colour with run_network's zero-embedding rule and frame features, output selection, no
side effects on the training state, and the NerfRunner methods built on it.

Allowances come from the reference side only (query_oracle.make_case): fp32 normals within 8x the
spread between the oracle in fp32 and the same composition with the MLP in float64; amp normals and
colours within the distance between the oracle's own amp and fp32 results. Errors are normalised per
point by |g_ref| + floor, floor = the set's mean |g_ref|: the error scales with the terms a gradient
is summed from, not with a gradient that happens to cancel. The measured figures are printed and
written to profiles/r8/query_field_parity.json when NOF_WRITE_PARITY is set."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import query_oracle as QO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PARITY = {}


@functools.lru_cache(maxsize=None)
def _case(name):
    return QO.make_case(name)


@functools.lru_cache(maxsize=None)
def _field(name, amp):
    from bundlesdf_amd.fused import FusedStep
    from bundlesdf_amd.grid import GridEncoder
    from bundlesdf_amd.nerf_helpers import FeatureArray, NeRFSmall, PoseArray
    c = _case(name)
    cfg, g, dev = c["cfg"], c["golden"], torch.device("cuda")
    L, n_ff = cfg["num_levels"], cfg.get("frame_features", 0)
    enc = GridEncoder(3, L, 2, cfg["base_res"], cfg["log2_hashmap_size"], cfg["finest_res"]).to(dev)
    enc.embeddings.data.copy_(c["emb"])
    net = NeRFSmall(2, 64, 15, 3, 64, input_ch=2 * L, input_ch_views=9 + n_ff).to(dev)
    net.load_state_dict(c["W"])
    pa = PoseArray(g["pose0"].shape[0], 0.1, 20.0).to(dev)
    fa = None
    if n_ff:
        fa = FeatureArray(g["pose0"].shape[0], n_ff).to(dev)
        fa.data.data.copy_(c["ff"])
    return FusedStep(cfg, torch.from_numpy(g["batch"]).to(dev), torch.from_numpy(g["c2w"]), torch.from_numpy(g["occ"]),
                     enc, net, pa, amp=amp, feature_array=fa)


@functools.lru_cache(maxsize=None)
def _all(name, amp, frame_id=0):
    r = _field(name, amp).query_field(_case(name)["pts"], sdf=True, normals=True, colour=True, frame_id=frame_id)
    return {k: v.cpu().numpy() for k, v in r.items()}


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


CASES = ["golden", "mixed"]
MODES = [pytest.param(True, id="amp"), pytest.param(False, id="fp32")]


@pytest.mark.parametrize("amp", MODES)
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("n", [1, 33, 3000])
def test_sdf_is_bit_identical_to_query_sdf(cuda_device, name, amp, n):
    """n = 1: a lone lane of a partial tile (each of the four kinds of point on its own); 33: a full
    tile plus one; 3000: several blocks and the grid-stride loop."""
    fs, pts = _field(name, amp), _case(name)["pts"]
    sets = [pts[i:i + 1] for i in range(4)] if n == 1 else [pts[:n]]
    for p in sets:
        want = fs.query_sdf(points=torch.from_numpy(p))
        for kw in (dict(), dict(normals=True), dict(normals=True, colour=True)):
            got = fs.query_field(p, **kw)["sdf"]
            assert got.shape == (len(p),) and torch.equal(got, want), kw
    if n == 3000:   # the launch chunks: the result does not depend on chunk
        a = fs.query_field(pts, normals=True, colour=True, chunk=1000)
        for k, v in _all(name, amp).items():
            assert np.array_equal(a[k].cpu().numpy(), v), k


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("n", [1, 33, 3000])
def test_normals_fp32_match_oracle(cuda_device, name, n):
    c = _case(name)
    ref, f64 = c[("fp32", 0)]["normal"].numpy(), c["f64"]["normal"].numpy()
    floor = float(np.linalg.norm(ref, axis=1).mean())
    allowance = 8 * QO.normalised(ref, f64, floor).max()
    fs = _field(name, False)
    if n == 1:
        got = np.concatenate([fs.query_field(c["pts"][i:i + 1], sdf=False, normals=True)["normals"].cpu().numpy()
                              for i in range(4)])
    else:
        got = fs.query_field(c["pts"][:n], sdf=False, normals=True)["normals"].cpu().numpy()
    err = QO.normalised(got, ref[:len(got)], floor).max()
    _record(f"normals_fp32/{name}/n{n}", gpu_max=err, allowance=allowance)
    assert err <= allowance, (err, allowance)


@pytest.mark.parametrize("name", CASES)
def test_normals_amp_match_oracle(cuda_device, name):
    """Set aside (query_oracle.kink_points): golden 0 %, mixed 6.4 % of the 3000 points (cap 10 %)."""
    c = _case(name)
    ref, f32 = c[("amp", 0)]["normal"].numpy(), c[("fp32", 0)]["normal"].numpy()
    kink, delta = QO.kink_points(c)
    assert kink.mean() <= 0.10, kink.mean()
    floor = float(np.linalg.norm(f32, axis=1).mean())
    allowance = QO.normalised(ref, f32, floor)[~kink].max()
    got = _all(name, True)["normals"]
    err = QO.normalised(got, ref, floor)[~kink].max()
    _record(f"normals_amp/{name}", gpu_max=err, allowance=allowance, set_aside=kink.mean(), kink_delta=delta)
    assert err <= allowance, (err, allowance)
    for n in (1, 33):   # the partial tiles give the same bits
        part = _field(name, True).query_field(c["pts"][:n], sdf=False, normals=True)["normals"].cpu().numpy()
        assert np.array_equal(part, got[:n])


@pytest.mark.parametrize("amp", MODES)
def test_clip_semantics(cuda_device, amp):
    """SDF and normal of a point outside the box are those of its clipped position, bit for bit."""
    fs = _field("mixed", amp)
    r = fs.query_field(np.array([[1.05, 0.2, -0.3], [1.0, 0.2, -0.3]], np.float32), normals=True)
    assert torch.equal(r["sdf"][0], r["sdf"][1]) and torch.equal(r["normals"][0], r["normals"][1])
    assert float(r["normals"][1].abs().max()) > 0


@pytest.mark.parametrize("name", CASES)
def test_colour_matches_oracle(cuda_device, name):
    c = _case(name)
    outside = (np.abs(c["pts"]) > 1).any(1)
    assert outside.sum() > 100
    ref = c[("fp32", 0)]["rgb"].numpy()
    got = _all(name, False)["colour"]
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5)
    # a point outside the box reads the colour of a ZERO embedding, which is not its clipped point's
    zero = QO.field_query(np.full((1, 3), 2.0, np.float32), c["emb"], *c["meta"], c["W"])["rgb"].numpy()
    np.testing.assert_allclose(got[outside], np.broadcast_to(zero, got[outside].shape), rtol=1e-4, atol=1e-5)
    clipped = _field(name, False).query_field(np.clip(c["pts"][outside], -1, 1), sdf=False, colour=True)
    assert np.abs(clipped["colour"].cpu().numpy() - got[outside]).max() > 1e-4


def test_colour_takes_the_frame_features(cuda_device):
    c = _case("mixed_ff")
    got = [_all("mixed_ff", False, fid)["colour"] for fid in (0, 1)]
    assert np.abs(got[0] - got[1]).max() > 1e-3
    for fid in (0, 1):
        np.testing.assert_allclose(got[fid], c[("fp32", fid)]["rgb"].numpy(), rtol=1e-4, atol=1e-5)
    amp = [_all("mixed_ff", True, fid)["colour"] for fid in (0, 1)]
    assert np.abs(amp[0] - amp[1]).max() > 1e-3
    with pytest.raises(RuntimeError, match="frame_id"):
        _field("mixed_ff", False).query_field(c["pts"][:4], colour=True, frame_id=3)


@pytest.mark.parametrize("amp", MODES)
def test_output_selection(cuda_device, amp):
    """Each non-empty subset of the outputs returns exactly its keys, bit-identical to the full call."""
    fs, pts, full = _field("mixed", amp), _case("mixed")["pts"], _all("mixed", amp)
    keys = ("sdf", "normals", "colour")
    for mask in range(1, 8):
        want = {k for i, k in enumerate(keys) if mask >> i & 1}
        r = fs.query_field(pts, sdf="sdf" in want, normals="normals" in want, colour="colour" in want)
        assert set(r) == want
        for k in want:
            assert np.array_equal(r[k].cpu().numpy(), full[k]), (mask, k)
    with pytest.raises(ValueError):
        fs.query_field(pts, sdf=False)
    empty = fs.query_field(np.zeros((0, 3), np.float32), normals=True, colour=True)
    assert empty["sdf"].shape == (0,) and empty["normals"].shape == (0, 3) and empty["colour"].shape == (0, 3)


@pytest.mark.parametrize("amp", MODES)
def test_query_leaves_the_training_state_alone(cuda_device, amp):
    """One captured step, the query, a second captured step: parameters, Adam state and loss_acc are
    untouched by the query, and the graph still replays the eager step (test_gpu_graph's comparison)."""
    import bench
    from bundlesdf_amd.fused import FusedStep
    dev = cuda_device
    cfg, pool, frame_start, c2w, occ, _, _ = bench.build_rank_scene(0, 1, 4, dict(amp=amp, n_step=40), dev)

    def trainer():
        enc, net, pa = bench.make_models(cfg, len(frame_start) - 1, dev)
        return FusedStep(cfg, pool, torch.from_numpy(c2w), occ, enc, net, pa, amp=amp, frame_start=frame_start)
    eager, graph = trainer(), trainer()
    pts = np.random.default_rng(3).uniform(-1.1, 1.1, (3000, 3)).astype(np.float32)
    for gs in range(2):
        oe = eager.step(ids=eager.sample_ids(512, 50 + gs), seed=3)
        og = graph.graph_step(512, seed_base=3, batch_seed_base=50)
        torch.testing.assert_close(og["loss_terms"][:6], oe["loss_terms"][:6], rtol=2e-3, atol=1e-6)
        assert torch.equal(graph.ids, eager.ids)
        if gs == 0:
            torch.cuda.synchronize()
            before = [t.clone() for t in (graph.P, graph.M, graph.V, graph.loss_acc)]
            r = graph.query_field(pts, normals=True, colour=True)
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(v).all()) for v in r.values())
            for b, t in zip(before, (graph.P, graph.M, graph.V, graph.loss_acc)):
                assert torch.equal(b, t)
    for name in ("P", "M", "V"):
        a, b = getattr(graph, name), getattr(eager, name)
        assert float((a - b).norm() / b.norm().clamp_min(1e-30)) < 4e-3, name


def test_runner_normals_colours_and_mesh_hook(cuda_device, tmp_path):
    from bundlesdf_amd import synthetic as SY
    from bundlesdf_amd.mesh import largest_component
    from bundlesdf_amd.nerf_runner import NerfRunner
    seq = SY.make_sequence(3, seed=2)
    cfg = SY.default_cfg(sc_factor=seq["sc_factor"], translation=seq["translation"], n_step=150, N_rand=2048,
                         num_levels=16, amp=True)
    cfg.update(save_dir=str(tmp_path / "plain"), mesh_resolution=0.004)
    nr = NerfRunner(cfg, seq["rgbs"], seq["depths"], seq["masks"], None, seq["poses"], seq["K"],
                    build_octree_pcd=seq["octree_pts"])
    nr.train()
    pts = torch.from_numpy(np.random.default_rng(0).uniform(-1.05, 1.05, (500, 3)).astype(np.float32))
    out, valid = nr.run_network_density(pts, get_normals=True)
    assert out.shape == (500, 4) and valid.shape == (500,) and bool(valid.all())
    assert torch.equal(out[:, :1], nr.run_network_density(pts)[0])
    assert torch.equal(out[:, 1:], nr.trainer.query_field(pts, sdf=False, normals=True)["normals"])
    # orientation: on the sphere part of the synthetic object the normal points outwards
    mesh = largest_component(nr.extract_mesh(voxel_size=0.004))
    assert nr.mesh_vertex_normals_from_network(mesh) is mesh and mesh.vertex_normals.shape == (len(mesh.vertices), 3)
    norm = np.linalg.norm(mesh.vertex_normals, axis=1)
    assert np.all((np.abs(norm - 1) < 1e-6) | (norm == 0))
    pw = mesh.vertices / seq["sc_factor"] - np.asarray(seq["translation"]).reshape(1, 3)
    d_sph = np.linalg.norm(pw, axis=1) - SY.SPHERE_R
    q = np.abs(pw - SY.BOX_C) - SY.BOX_H
    d_box = np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(1), 0)
    on_sphere = (np.abs(d_sph) < 2e-3) & (d_box > 5e-3)
    assert on_sphere.sum() > 100
    dots = (mesh.vertex_normals[on_sphere] * (pw[on_sphere] / np.linalg.norm(pw[on_sphere], axis=1, keepdims=True))).sum(1)
    print(f"sphere vertices {on_sphere.sum()}, outward share {np.mean(dots > 0):.3f}")
    assert np.mean(dots > 0) >= 0.95
    assert nr.mesh_vertex_color_from_network(mesh) is mesh
    rgb = nr.trainer.query_field(mesh.vertices.astype(np.float32), sdf=False, colour=True)["colour"].cpu().numpy()
    assert mesh.vertex_colors.dtype == np.uint8 and mesh.vertex_colors.shape == (len(mesh.vertices), 3)
    assert np.array_equal(mesh.vertex_colors, (rgb * 255).astype(np.uint8))
    # the mesh hook: attributes only when asked for, otherwise the plain export of the same mesh
    nr._hook_mesh()
    name = f"step_{nr.global_step:07d}_mesh_normalized_space.obj"
    plain = nr.extract_mesh(isolevel=0, voxel_size=cfg["mesh_resolution"])
    plain.export(str(tmp_path / "expect.obj"))
    assert open(tmp_path / "plain" / name, "rb").read() == open(tmp_path / "expect.obj", "rb").read()
    nr.cfg["mesh_vertex_attributes"] = True
    nr.cfg["save_dir"] = str(tmp_path / "attr")
    nr._hook_mesh()
    lines = open(tmp_path / "attr" / name).read().split("\n")
    v = [ln for ln in lines if ln.startswith("v ")]
    assert len(v) == len(plain.vertices) and all(len(ln.split()) == 7 for ln in v)
    assert sum(ln.startswith("vn ") for ln in lines) == len(v)
    assert all("//" in ln for ln in lines if ln.startswith("f "))


@pytest.mark.parametrize("name,fid", [("golden", 0), ("mixed", 0), ("mixed_ff", 0), ("mixed_ff", 1)])
def test_colour_amp_within_oracle_distance(cuda_device, name, fid):
    """amp colour against the oracle's amp colour, allowance = the oracle's own amp-vs-fp32 distance on
    the same points (normalised as the normals are). That distance is about half an fp16 ulp of a colour
    logit, so the kernel's colour pass has to round where autocast rounds: with the training forward's
    features (one rounding after the fp32 sum) and fp32 bias it is 1.42e-05 against 1.08e-05 (golden)
    and 1.77e-05 against 1.47e-05 (mixed); k_query_field's colour pass sums its features as the half
    kernel does and adds the bias rounded to fp16."""
    c = _case(name)
    ref, f32 = c[("amp", fid)]["rgb"].numpy(), c[("fp32", fid)]["rgb"].numpy()
    floor = float(np.linalg.norm(f32, axis=1).mean())
    allowance = QO.normalised(ref, f32, floor).max()
    err = QO.normalised(_all(name, True, fid)["colour"], ref, floor).max()
    _record(f"colour_amp/{name}/frame{fid}", gpu_max=err, allowance=allowance)
    assert err <= allowance, (err, allowance)
