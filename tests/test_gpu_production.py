"""The production instances of the fused step against the oracle, tile by tile.

nof_field_step compiles its forward kernels twice: k_encode<.., DBG = true> / k_colour<.., true>
run when a dbg_* pointer is set (FusedStep.step(debug=True), what every other oracle or golden
parity test calls), the DBG = false instances otherwise (bench.py, NerfRunner.train, every graph
replay). The debug k_encode forces the colour net onto every tile, so it writes only tile flags 1
and 3: the sigma-only backward (flag 2, k_compact's back list with bit 31, the sigma-only branch of
k_mlp_bwd), the tiles with valid samples and no work (flag 0), the early exit of a tile without a
valid sample, k_scatter's and k_ray_final's flag gates are reached by the production instances alone.

Each test here re-runs one existing parity case of test_gpu_step.py with debug=False, on the same
inputs and with the same tolerances, and reads the production step's results without any debug
output: the gradient buffers and loss accumulators in a grad_hook (after the backward, before the
optimiser), FusedStep.tile_counters() and the tile flags / lists after the step. A debug twin (a
second FusedStep from the same initial state, debug=True, same ids and draws) supplies the z /
validity / sdf records aligned_ref and mask_flips need — the production k_encode computes the same
values with the same arithmetic — and its counters state why it does not cover production:
records_sigma == 0 and tiles_colour == every tile.

The tile classes come from the oracle's records through tests/tile_oracle.py (the loss definitions,
float64), not from the kernel: the production step's four counters, every tile flag and the three
tile lists must equal them — exactly on inputs without a loss-mask flip, within n tiles with n
flips (a flipped sample can move its tile to another class; aligned_ref caps n at FLIP_MAX).

Inputs. No seed of _scene_case (0 .. 48 tried) or _ff_case (11 .. 20) has a sample outside the box,
and the ray pool holds rays of type 0 only, so the config-2 case gets a second, smaller variant
("config2_offbox": _scene_case(seed 0, R = 128) with every 16th ray's depth moved to 0.95 far —
its around-depth band lies outside the box: two tiles without a valid sample per ray — and every
16th ray + 5 set to type 1 inside its band: colour tiles with no backward, flag 3).
test_production_cases_cover_every_tile_class checks the conditions on the oracle's records alone."""
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

from oracle import nerf_step as NS
from tests import tile_oracle as TO
from tests.test_gpu_step import (_METRICS, AMP_LOSS_TOL, AMP_SHAPES_G4, EDGE_CASES, G4AMP_TABLE_KAPPA, KAPPA_AMP,
                                 SHAPES, _build, _check_all, _ff_case, _ff_fused, _scene_case, _shape,
                                 _write_metrics, aligned_ref, mask_flips)  # noqa: F401  (_write_metrics: fixture)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FF_KEYS = ["embeddings", "pose", "features"] + NS.MLP_KEYS
SIGMA_ONLY_MIN = 50      # sigma-only backward tiles each of the cases 1-4 must hold
# tile flag k_encode writes for each tile_oracle class: invalid 0, colour + backward 1, sigma-only 2,
# colour forward-only 3, valid without work 0
CLASS_FLAG = np.array([0, 1, 2, 3, 0], np.uint8)


def _production_step(fs, ids, t_rand):
    """One step(debug=False) — the production kernel instances — and what it computed: the loss
    accumulators and the unscaled flat gradient cloned in a grad_hook (the table gradient is G16 in
    amp; every scale used here is a power of two, so the division is exact), split like the
    oracle's params, and the work counters."""
    got = {}

    def hook(f):
        G = f.G.clone()
        if f.amp:
            G[:f.n_emb] = f.G16.float()
            G /= f.scale
        got.update(G=G, loss=f.loss_acc.clone())

    out = fs.step(ids=ids, t_rand=t_rand, debug=False, grad_hook=hook)
    torch.cuda.synchronize()
    assert "dbg" not in out and "grads" not in out
    loss = got["loss"].cpu().numpy().astype(np.float64)
    return types.SimpleNamespace(loss_terms=loss[:8], fs_rgb_loss=float(loss[140]), G=fs.split(got["G"].cpu()),
                                 counters=fs.tile_counters())


def _oracle_once(fn):
    """fn() computed once and kept (the production test, its shapes and the classifier share it,
    unchanged); a call with arguments (aligned_ref's mask_from) runs the oracle again."""
    box = {}

    def call(**kw):
        if kw:
            return fn(**kw)
        if "ref" not in box:
            box["ref"] = fn()
        return box["ref"]
    return call


def _golden_case(fname, amp):
    g = np.load(os.path.join(GOLDEN, fname))
    cfg = json.loads(str(g["cfg_json"]))
    mlp_w = {k: g["w0_" + k] for k in NS.MLP_KEYS}
    scale = float(g["loss_scale"][0]) if amp else None

    def make(dev):
        from bundlesdf_amd.fused import FusedStep
        enc, net, pa = _build(dev, cfg, g["emb0"], mlp_w, g["pose0"], cfg["num_levels"], cfg["log2_hashmap_size"],
                              cfg["finest_res"])
        fs = FusedStep(cfg, torch.from_numpy(g["batch"]).to(dev), torch.from_numpy(g["c2w"]),
                       torch.from_numpy(g["occ"]), enc, net, pa, amp=amp)
        if amp:
            fs.scale.fill_(scale)
        return fs

    def oracle():
        # the reference's own gradients (the golden) with the oracle's conditioning on the same inputs,
        # as test_fused_step_matches_reference_train_loop / .._amp_.. build it
        P0 = {"embeddings": torch.from_numpy(g["emb0"]), "pose": torch.from_numpy(g["pose0"])}
        P0.update({k: torch.from_numpy(g["w0_" + k]) for k in NS.MLP_KEYS})
        meta = (g["offsets"], float(np.log2(g["per_level_scale"][0])), cfg["base_res"])
        kw = dict(amp=True, loss_scale=scale) if amp else {}
        o = NS.train_step(P0, torch.from_numpy(g["batch"]), torch.from_numpy(g["c2w"]), g["occ"], cfg,
                          torch.from_numpy(g["t_rand"]), meta, **kw)
        widen = 1.0 + G4AMP_TABLE_KAPPA / KAPPA_AMP if amp else 1.0
        ref = {"grads": {"embeddings": torch.from_numpy(g["g_emb"]), "pose": torch.from_numpy(g["g_pose"])},
               "g_emb_abs": o["g_emb_abs"] * widen, "g_emb_dpos": o["g_emb_dpos"], "g_mlp_abs": o["g_mlp_abs"],
               "g_mlp_kink": o["g_mlp_kink"], "g_emb_kink": o["g_emb_kink"],
               "z_vals": torch.from_numpy(g["z_vals"]), "raw": torch.from_numpy(g["raw"]),
               "valid": torch.from_numpy(g["valid"]), "loss": float(g["loss"])}
        ref["grads"].update({k: torch.from_numpy(g["g_" + k]) for k in NS.MLP_KEYS})
        return ref

    return types.SimpleNamespace(cfg=cfg, batch=g["batch"], t_rand=g["t_rand"], amp=amp, make=make,
                                 oracle=_oracle_once(oracle), keys=None, golden=g)


def _scene(cfg, seq, batch, occ, t_rand, mlp_w, emb, pose, offs, amp=False, scale=None, ff=None, grid=(22, 128)):
    c2w = torch.from_numpy(np.asarray(seq["poses"], np.float32))
    from bundlesdf_amd.grid import level_layout
    pls, _ = level_layout(3, 16, 2, 16, *grid)

    def make(dev):
        from bundlesdf_amd.fused import FusedStep
        if ff is not None:
            fs, _ = _ff_fused(dev, cfg, seq, batch, occ, mlp_w, emb, pose, ff, amp=amp)
        else:
            enc, net, pa = _build(dev, cfg, emb, mlp_w, pose, 16, *grid)
            fs = FusedStep(cfg, torch.from_numpy(batch).to(dev), c2w, torch.from_numpy(occ), enc, net, pa, amp=amp)
        if scale is not None:
            fs.scale.fill_(scale)
        return fs

    def oracle(**kw):
        P0 = {"embeddings": torch.from_numpy(emb), "pose": torch.from_numpy(pose)}
        if ff is not None:
            P0["features"] = torch.from_numpy(ff)
        P0.update({k: torch.from_numpy(v) for k, v in mlp_w.items()})
        if amp:
            kw = dict(kw, amp=True, loss_scale=scale)
        return NS.train_step(P0, torch.from_numpy(batch), c2w, occ, cfg, torch.from_numpy(t_rand),
                             (offs, float(np.log2(pls)), 16), **kw)

    return types.SimpleNamespace(cfg=cfg, batch=batch, t_rand=t_rand, amp=amp, make=make, oracle=_oracle_once(oracle),
                                 keys=None if ff is None else FF_KEYS, golden=None)


def _edge_inputs(case):
    """The inputs of test_fused_step_ragged_and_empty_batches_match_oracle."""
    R, seed = EDGE_CASES[case]["R"], EDGE_CASES[case]["seed"]
    cfg, seq, batch, occ, t_rand, mlp_w, emb, pose, offs = _scene_case(seed=seed, R=R)
    batch = batch.copy()
    if case == "single":
        sc = cfg["sc_factor"]
        ok = np.nonzero((batch[:, 9] == 0) & (batch[:, 7] > 0) & (batch[:, 6] > cfg["near"] * sc) &
                        (batch[:, 6] < cfg["far"] * sc))[0]
        batch, t_rand = batch[ok[:1]].copy(), t_rand[ok[:1]].copy()
    if case == "mixed45":
        batch[1::3, 9] = 1.0
        batch[2::5, 6] = 2.0 * cfg["far"] * cfg["sc_factor"]
    if case == "no_backward64":
        batch[:, 9] = 1.0
    return cfg, seq, batch, occ, t_rand, mlp_w, emb, pose, offs


@functools.lru_cache(maxsize=None)
def _case(name):
    """The inputs of one parity case, a factory of FusedSteps in its initial state, and its oracle
    step (computed once)."""
    if name == "g4":
        return _golden_case("train_step.npz", False)
    if name == "g4amp":
        return _golden_case("train_step_amp.npz", True)
    if name == "config2":
        return _scene(*_scene_case())
    if name == "config2_offbox":
        cfg, seq, batch, *rest = _scene_case(R=128)
        batch = batch.copy()
        batch[::16, 6] = 0.95 * cfg["far"] * cfg["sc_factor"]   # the around-depth band lies outside the box
        batch[5::16, 9] = 1.0                                   # type-1 rays composite colour, carry no loss
        return _scene(cfg, seq, batch, *rest)
    if name == "ff_amp":
        cfg, seq, batch, occ, t_rand, mlp_w, emb, pose, offs, ff = _ff_case(seed=13)
        cfg["amp"] = True
        # scale 1024: the case's fp16 weight gradients overflow at 2^16 (the step would skip)
        return _scene(cfg, seq, batch, occ, t_rand, mlp_w, emb, pose, offs, amp=True, scale=1024.0, ff=ff,
                      grid=(19, 512))
    if name == "fs_rgb":
        cfg, *rest = _scene_case(seed=23)
        cfg["fs_rgb_weight"] = 10.0
        return _scene(cfg, *rest)
    kind, case, mode = name.split(":")
    assert kind == "edge"
    cfg, *rest = _edge_inputs(case)
    cfg["amp"] = mode == "amp"
    return _scene(cfg, *rest, amp=mode == "amp", scale=1024.0 if mode == "amp" else None)


def _classes(c, ref):
    return TO.classify_tiles(c.batch, ref["z_vals"], ref["raw"][..., 3], ref["valid"], c.cfg, NS.truncation(c.cfg))


_ALIGNED = {}


def _aligned(prefix, name, c, dbg):
    """aligned_ref on the case's cached oracle step; the re-run on the kernels' branches (only with
    flips) is kept per case and (z, sdf), which every scatter shape of a case shares. Returns the
    reference and the flip count."""
    def ref_fn(**kw):
        if not kw:
            return c.oracle()
        key = (name,) + tuple(hash(t.numpy().tobytes()) for t in kw["mask_from"])
        if key not in _ALIGNED:
            _ALIGNED[key] = c.oracle(**kw)
        return _ALIGNED[key]
    ref = aligned_ref(prefix, dbg, ref_fn, c.batch, c.cfg, NS.truncation(c.cfg))
    return ref, int(_METRICS[f"{prefix}/mask_flips"])


def _run(dev, name, shape=None):
    """The case's debug twin and its production step, both from the initial state on the same ids
    and draws. The twin's counters must show that it ran the colour net on every tile and no
    sigma-only backward record."""
    c = _case(name)
    R, S = c.t_rand.shape
    ids = torch.arange(R, dtype=torch.int32, device=dev)
    t_rand = torch.from_numpy(c.t_rand)
    twin = c.make(dev)
    if shape is not None:
        _shape(twin, shape)
    dbg = twin.step(ids=ids, t_rand=t_rand, debug=True)["dbg"]
    torch.cuda.synchronize()
    tc = twin.tile_counters()
    assert tc["records_sigma"] == 0 and tc["tiles_colour"] == R * S // 32, tc
    fs = c.make(dev)
    if shape is not None:
        _shape(fs, shape)
    return c, dbg, fs, _production_step(fs, ids, t_rand)


def _check_tiles(prefix, fs, prod, cls, flips):
    """The production step's work counters, tile flags and tile lists against the oracle's classes:
    exact without a loss-mask flip, within `flips` tiles otherwise."""
    want = TO.counters(cls)
    for k, v in want.items():
        short = k.replace("tiles_", "")
        _METRICS[f"{prefix}/tiles_{short}"] = prod.counters[k]
        _METRICS[f"{prefix}/tiles_{short}_want"] = v
    for k, v in want.items():
        assert abs(prod.counters[k] - v) <= flips, (k, prod.counters, want, flips)
    offs, nt = fs._ws_offsets()
    assert nt == cls.size
    flags = fs.workspace[offs["tile_bwd"]:offs["tile_bwd"] + nt].cpu().numpy()
    wrong = np.nonzero(flags != CLASS_FLAG[cls.ravel()])[0]
    assert wrong.size <= flips, (f"{prefix}: {wrong.size} tile flags differ from the oracle's classes, first tile "
                                 f"{wrong[:8]}: got {flags[wrong[:8]]}, class {cls.ravel()[wrong[:8]]}")
    # the lists k_compact wrote hold exactly the flagged tiles: colour-backward entries in front, the
    # sigma-only ones behind with bit 31 (tile_lists checks the halves), the colour tiles in their own list
    bl, cl = fs.tile_lists()
    bl, cl = bl.cpu().numpy(), cl.cpu().numpy()
    np.testing.assert_array_equal(np.sort((bl[bl < 0] & 0x7fffffff) >> 5), np.nonzero(flags == 2)[0])
    np.testing.assert_array_equal(bl[bl >= 0] >> 5, np.nonzero(flags == 1)[0])
    np.testing.assert_array_equal(cl >> 5, np.nonzero((flags == 1) | (flags == 3))[0])
    assert fs.n_tile_records() == int(((flags == 1) | (flags == 2)).sum())


COVER = ["g4", "g4amp", "config2", "ff_amp", "config2_offbox", "fs_rgb"]


def test_production_cases_cover_every_tile_class(cuda_device):
    """Conditions on the inputs, from the oracle's records alone (the device only builds the ray
    pool): every tile class occurs, each of the cases 1-4 holds at least SIGMA_ONLY_MIN sigma-only
    backward tiles, config2_offbox holds tiles without a valid sample and a ray of type != 0 with
    samples inside the band (colour tiles with no backward), and no tile's class hinges on a band
    residual another float32 implementation may see as an exact zero."""
    total = dict.fromkeys(TO.CLASS_NAMES, 0)
    for name in COVER:
        c = _case(name)
        ref = c.oracle()
        trunc = NS.truncation(c.cfg)
        sdf = ref["raw"][..., 3]
        n = TO.class_counts(_classes(c, ref))
        for k, v in n.items():
            total[k] += v
            _METRICS[f"prod_{name}/classes/{k}"] = v
        assert TO.hinge_tiles(c.batch, ref["z_vals"], sdf, ref["valid"], c.cfg, trunc) == 0, name
        if name in COVER[:4]:
            assert n["sigma_bwd"] >= SIGMA_ONLY_MIN, (name, n)
        if name == "config2_offbox":
            assert n["invalid"] >= 1 and n["colour_fwd"] >= 1, n
            assert TO.rays_with_band_samples(c.batch, ref["z_vals"], ref["valid"], c.cfg, trunc) >= 1
    assert all(v >= 1 for v in total.values()), total


@pytest.mark.parametrize("shape", list(SHAPES))
def test_production_step_matches_reference_train_loop(cuda_device, shape):
    """G4 (tests/golden/train_step.npz), fp32: loss, every gradient entry and the parameters after
    Adam of the production step against the reference's own train_loop."""
    c, dbg, fs, prod = _run(cuda_device, "g4", shape)
    g, ref = c.golden, c.oracle()
    prefix = f"prod_g4_{shape}"
    flips = mask_flips(dbg, ref, c.batch, c.cfg, NS.truncation(c.cfg))
    _METRICS[f"{prefix}/mask_flips"] = flips
    assert flips == 0
    np.testing.assert_allclose(prod.loss_terms[:4].sum(), ref["loss"], rtol=1e-4)
    _check_all(prefix, prod.G, ref)
    _check_tiles(prefix, fs, prod, _classes(c, ref), 0)
    P = fs.split(fs.P.detach().cpu())
    np.testing.assert_allclose(P["embeddings"].numpy(), g["emb1"], atol=2e-5)
    for k in NS.MLP_KEYS:
        np.testing.assert_allclose(P[k].numpy(), g["w1_" + k], atol=2e-5, err_msg=k)
    np.testing.assert_allclose(P["pose"].numpy(), g["pose1"], atol=2e-5)


@pytest.mark.parametrize("shape", list(AMP_SHAPES_G4))
def test_production_step_amp_matches_reference_amp_train_loop(cuda_device, shape):
    """G4-amp (tests/golden/train_step_amp.npz, the fixture's loss scale): the allowances of
    test_fused_step_amp_matches_reference_amp_train_loop, G4AMP_TABLE_KAPPA included."""
    c, dbg, fs, prod = _run(cuda_device, "g4amp", shape)
    ref = c.oracle()
    prefix = f"prod_g4amp_{shape}"
    flips = mask_flips(dbg, ref, c.batch, c.cfg, NS.truncation(c.cfg))
    _METRICS[f"{prefix}/mask_flips"] = flips
    assert flips == 0, f"{flips} samples on the other side of a loss-mask threshold than the reference"
    loss = float(prod.loss_terms[:4].sum())
    _METRICS[f"{prefix}/loss"] = abs(loss - ref["loss"]) / ref["loss"]
    np.testing.assert_allclose(loss, ref["loss"], rtol=AMP_LOSS_TOL)
    _check_all(prefix, prod.G, ref, amp=True)
    _check_tiles(prefix, fs, prod, _classes(c, ref), 0)


@pytest.mark.parametrize("name,shape", [("config2", s) for s in SHAPES] + [("config2_offbox", "split")])
def test_production_step_matches_oracle_config2(cuda_device, name, shape):
    """The config-2 scene (L = 16, 2^22 table, 192 samples per ray), fp32, and its variant with tiles
    that hold no valid sample and type-1 rays inside the band (module docstring)."""
    c, dbg, fs, prod = _run(cuda_device, name, shape)
    prefix = f"prod_{name}_{shape}"
    ref, flips = _aligned(prefix, name, c, dbg)
    np.testing.assert_allclose(prod.loss_terms[:4].sum(), ref["loss"], rtol=1e-4)
    _check_all(prefix, prod.G, ref)
    _check_tiles(prefix, fs, prod, _classes(c, ref), flips)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_production_step_frame_features_amp_matches_oracle_amp(cuda_device, shape):
    """Frame features, amp (BASELINE config 5's numerics: S = 320, hashed top levels, scale 1024): the
    n_ff > 0 instance of the MLP backward's first pass with sigma-only tiles in its list."""
    c, dbg, fs, prod = _run(cuda_device, "ff_amp", shape)
    prefix = f"prod_ff_amp_{shape}"
    ref, flips = _aligned(prefix, "ff_amp", c, dbg)
    assert all(torch.isfinite(v).all() for v in ref["grads"].values())
    assert c.t_rand.shape[1] == 320
    lt = prod.loss_terms
    for k, got in (("rgb_loss", lt[0]), ("fs_loss", lt[1] + lt[2]), ("sdf_loss", lt[3])):
        _METRICS[f"{prefix}/{k}"] = abs(got - ref[k]) / abs(ref[k])
        np.testing.assert_allclose(got, ref[k], rtol=AMP_LOSS_TOL, err_msg=k)
    np.testing.assert_allclose(lt[6], ref["reg_features"], rtol=1e-5)
    _check_all(prefix, prod.G, ref, keys=FF_KEYS, amp=True)
    _check_tiles(prefix, fs, prod, _classes(c, ref), flips)


def test_production_fs_rgb_loss_matches_oracle(cuda_device):
    """cfg fs_rgb_weight > 0: the front tiles that would be sigma-only run the colour net and its
    backward (the case has no sigma-only tile left); the checks of test_fs_rgb_loss_matches_oracle."""
    c, dbg, fs, prod = _run(cuda_device, "fs_rgb")
    ref = c.oracle()
    assert ref["fs_rgb_loss"] > 0
    flips = mask_flips(dbg, ref, c.batch, c.cfg, NS.truncation(c.cfg))
    _METRICS["prod_fs_rgb/mask_flips"] = flips
    assert flips == 0
    np.testing.assert_allclose(prod.fs_rgb_loss, ref["fs_rgb_loss"], rtol=1e-4)   # unweighted metric
    np.testing.assert_allclose(prod.loss_terms[:4].sum() + 10.0 * prod.fs_rgb_loss, ref["loss"], rtol=1e-4)
    _check_all("prod_fs_rgb", prod.G, ref)
    cls = _classes(c, ref)
    plain = TO.classify_tiles(c.batch, ref["z_vals"], ref["raw"][..., 3], ref["valid"], dict(c.cfg, fs_rgb_weight=0),
                              NS.truncation(c.cfg))
    moved = int(((plain == TO.SIGMA_BWD) & (cls == TO.COLOUR_BWD)).sum())
    assert moved >= SIGMA_ONLY_MIN, moved     # the term is what makes these tiles colour tiles
    _check_tiles("prod_fs_rgb", fs, prod, cls, 0)


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_production_step_ragged_and_empty_batches_match_oracle(cuda_device, case, amp):
    """The ragged and empty batches of test_fused_step_ragged_and_empty_batches_match_oracle: the
    production k_encode's waves past the last tile, a single ray, type-1 rays and depths beyond far
    mixed in, and a batch without any loss-carrying ray (no list entry, every gradient exactly zero)."""
    mode = "amp" if amp else "fp32"
    name = f"edge:{case}:{mode}"
    c, dbg, fs, prod = _run(cuda_device, name)
    prefix = f"prod_edge_{case}_{mode}"
    ref, flips = _aligned(prefix, name, c, dbg)
    lt = prod.loss_terms
    assert np.isfinite(lt).all()
    for k, got in (("rgb_loss", lt[0]), ("fs_loss", lt[1] + lt[2]), ("sdf_loss", lt[3])):
        np.testing.assert_allclose(got, float(ref[k]), rtol=AMP_LOSS_TOL if amp else 1e-4, atol=1e-9, err_msg=k)
    _check_tiles(prefix, fs, prod, _classes(c, ref), flips)
    if case == "no_backward64":
        assert float(ref["loss"]) == 0.0
        for k, g in prod.G.items():
            assert int(torch.count_nonzero(g)) == 0, k
        assert fs.n_tile_records() == 0
        assert prod.counters["records_colour"] == 0 and prod.counters["records_sigma"] == 0
        return
    assert float(ref["loss"]) > 0 and int(torch.count_nonzero(ref["grads"]["embeddings"])) > 0
    assert int(torch.count_nonzero(prod.G["embeddings"])) > 0
    _check_all(prefix, prod.G, ref, amp=amp)


@pytest.mark.parametrize("debug", [False, True], ids=["production", "debug"])
def test_empty_batch_is_a_step_without_work(cuda_device, debug):
    """R = 0: no kernel of the field pass runs, in either instance — zero loss terms and counters,
    zero gradients, parameters unchanged by the optimiser."""
    c = _case("g4")
    fs = c.make(cuda_device)
    P0 = fs.P.detach().clone()
    S = c.t_rand.shape[1]
    ids = torch.zeros(0, dtype=torch.int32, device=cuda_device)
    got = {}
    out = fs.step(ids=ids, t_rand=torch.zeros(0, S), debug=debug, grad_hook=lambda f: got.update(G=f.G.clone()))
    torch.cuda.synchronize()
    assert float(out["loss_terms"].abs().sum()) == 0.0
    assert int(torch.count_nonzero(got["G"])) == 0
    assert fs.tile_counters() == dict(tiles_sigma=0, tiles_colour=0, records_colour=0, records_sigma=0)
    assert torch.equal(fs.P, P0)
