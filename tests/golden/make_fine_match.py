"""Record tests/golden/fine_match*.npz: what the reference's own FinePreprocess, LocalFeatureTransformer
(loftr_fine) and FineMatching give on the cases of tests/fine_oracle.py.

    python tests/golden/make_fine_match.py /path/to/the/reference/checkout

loftr_module/fine_preprocess.py (torch and einops) and loftr_module/transformer.py are loaded as
make_feature_transformer.py loads its modules. utils/fine_matching.py is loaded by file path too, but
it imports kornia, which need not be installed: before the load this script puts stand-ins of its own
into sys.modules, a few lines each for kornia.geometry.subpix.dsnt.spatial_expectation2d and
kornia.utils.grid.create_meshgrid (below). So the fixture pins the module's own code (the centre row,
the temperature, the variance, the clamp, get_fine_match's scaling), and the two kornia functions only
as restated here: the expectation of a heat map over a grid of x, y in linspace(-1, 1, W), x fastest.

The reference batches by pair; a frame shared between pairs is given to it once per pair
(fine[frames]). Weights come from fine_oracle's seeded generator and are not stored. Inputs are gain
times a seeded standard normal, rounded to fp16; the gain is raised from 1 in steps of sqrt(2) until
on the reference itself, on the CPU,
    the float64 (x, y) has an rms of at least 0.1: the heat maps are neither flat nor saturated, and
    the largest fp16-autocast error of (x, y) is below 1/20 of that rms,
so that a wrong axis order, window offset or centre row is many bounds away. Per case the fixture (cut
into shards below 1 MiB) holds, in float64,
    gain, fine_a, fine_b, coarse_a, coarse_b      the inputs
    win_a, win_b                                  FinePreprocess' two outputs
    expec_f, mkpts1_f                             FineMatching's
    {win,expec_f,mkpts1_f}_e16_{rms,max}          the reference's own half-precision error: its output under
                                                  torch.autocast("cpu", dtype=torch.float16) minus float64
    xy_rms, xy_e16_max                            the two figures of the conditions above
Data only, none of the reference's code.
"""
import importlib
import importlib.util
import os
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(directory, module, alias):
    pkg = types.ModuleType(alias)
    pkg.__path__ = [directory]
    sys.modules[alias] = pkg
    return importlib.import_module(f"{alias}.{module}")


def _meshgrid(h, w, normalized_coordinates=True, device=None, dtype=torch.float32):
    """[1,h,w,2] of (x, y): the pixel index, or linspace(-1, 1) along each axis."""
    xs = torch.linspace(0, w - 1, w, device=device, dtype=dtype)
    ys = torch.linspace(0, h - 1, h, device=device, dtype=dtype)
    if normalized_coordinates:
        xs, ys = (xs / (w - 1) - 0.5) * 2, (ys / (h - 1) - 0.5) * 2
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    return torch.stack([gx, gy], -1)[None]


def _spatial_expectation2d(heat, normalized_coordinates=True):
    """heat [B,N,H,W] (each map sums to 1) -> [B,N,2]: sum heat x, sum heat y."""
    B, N, H, Wd = heat.shape
    g = _meshgrid(H, Wd, normalized_coordinates, heat.device, heat.dtype).reshape(-1, 2)
    return heat.reshape(B, N, -1) @ g


def _stand_in_kornia():
    names = ("kornia", "kornia.geometry", "kornia.geometry.subpix", "kornia.geometry.subpix.dsnt", "kornia.utils",
             "kornia.utils.grid")
    mods = {n: types.ModuleType(n) for n in names}
    for n in names:
        if "." in n:
            setattr(mods[n.rsplit(".", 1)[0]], n.rsplit(".", 1)[1], mods[n])
    mods["kornia.geometry.subpix.dsnt"].spatial_expectation2d = _spatial_expectation2d
    mods["kornia.utils.grid"].create_meshgrid = _meshgrid
    sys.modules.update(mods)


def _by_path(path, alias):
    spec = importlib.util.spec_from_file_location(alias, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_reference(mods, O, case, w, inputs, dtype, autocast):
    """(win_a, win_b, expec_f, mkpts1_f) of the reference's three modules as float64 arrays."""
    FP, T, FM = mods
    c = O.CASES[case]
    pair, i, j, _ = O.case_matches(case)
    (h0, w0), (h1, w1), s = c["hw_a"], c["hw_b"], c["stride"]
    cfg = dict(fine_concat_coarse_feat=True, fine_window_size=O.W, coarse=dict(d_model=O.CC), fine=dict(d_model=O.C))
    pre = FP.FinePreprocess(cfg).eval()
    pre.load_state_dict({k[len("fine_preprocess."):]: torch.from_numpy(v) for k, v in w.items()
                         if k.startswith("fine_preprocess.")}, strict=True)
    net = T.LocalFeatureTransformer(dict(d_model=O.C, nhead=8, layer_names=list(O.LAYERS), attention="linear")).eval()
    net.load_state_dict({k[len("loftr_fine."):]: torch.from_numpy(v) for k, v in w.items() if k.startswith("loftr_fine.")},
                        strict=True)
    head = FM.FineMatching().eval()
    pre, net = pre.to(dtype), net.to(dtype)
    fa, fb, ca, cb = (torch.from_numpy(x).to(dtype) for x in inputs)
    fr_a = np.arange(c["P"]) if c["frames_a"] is None else np.asarray(c["frames_a"])
    fr_b = np.arange(c["P"]) if c["frames_b"] is None else np.asarray(c["frames_b"])
    scale_c = float(s * O.SCALE_F)
    tj = torch.from_numpy(j.astype(np.int64))
    data = dict(hw0_i=(O.SCALE_F * s * h0, O.SCALE_F * s * w0), hw1_i=(O.SCALE_F * s * h1, O.SCALE_F * s * w1),
                hw0_f=(s * h0, s * w0), hw1_f=(s * h1, s * w1), hw0_c=(h0, w0), hw1_c=(h1, w1),
                b_ids=torch.from_numpy(pair.astype(np.int64)), i_ids=torch.from_numpy(i.astype(np.int64)), j_ids=tj,
                mconf=torch.ones(len(pair), dtype=dtype))
    ti = data["i_ids"]
    data["mkpts0_c"] = torch.stack([ti % w0, ti // w0], 1).to(dtype) * scale_c          # get_coarse_match
    data["mkpts1_c"] = torch.stack([tj % w1, tj // w1], 1).to(dtype) * scale_c
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.float16, enabled=autocast):
        win_a, win_b = pre(fa[fr_a], fb[fr_b], ca, cb, data)
        f0, f1 = net(win_a, win_b)
        head(f0, f1, data)
    return tuple(t.double().numpy() for t in (win_a, win_b, data["expec_f"], data["mkpts1_f"]))


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    loftr = os.path.join(sys.argv[1], "BundleTrack", "LoFTR", "src", "loftr")
    FP = _load(os.path.join(loftr, "loftr_module"), "fine_preprocess", "reference_loftr_module")
    T = importlib.import_module("reference_loftr_module.transformer")
    _stand_in_kornia()
    FM = _by_path(os.path.join(loftr, "utils", "fine_matching.py"), "reference_fine_matching")
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tests import fine_oracle as O

    rms = lambda e: float(np.sqrt(np.mean(np.square(e))))
    rec = {}
    for case, c in O.CASES.items():
        w = O.make_weights(c["seed"])
        gain = 1.0
        for _ in range(12):
            inputs = O.make_inputs(case, gain)
            r64 = run_reference((FP, T, FM), O, case, w, inputs, torch.float64, False)
            r16 = run_reference((FP, T, FM), O, case, w, inputs, torch.float32, True)
            xy_rms = rms(r64[2][:, :2])
            xy_e16 = float(np.abs(r16[2][:, :2] - r64[2][:, :2]).max())
            print(f"{case}: gain {gain:.3f}  xy rms {xy_rms:.3f}  xy e16 max {xy_e16:.3e}")
            if xy_rms >= 0.1 and xy_e16 < xy_rms / 20:
                break
            gain *= np.sqrt(2.0)
        assert xy_rms >= 0.1 and xy_e16 < xy_rms / 20, (case, xy_rms, xy_e16)
        assert all(np.isfinite(x).all() for x in r16)
        rec[f"{case}_gain"] = np.float64(gain)
        for k, v in zip(("fine_a", "fine_b", "coarse_a", "coarse_b"), inputs):
            rec[f"{case}_{k}"] = v.astype(np.float64)
        for k, v in zip(("win_a", "win_b", "expec_f", "mkpts1_f"), r64):
            rec[f"{case}_{k}"] = v
        errs = dict(win=np.concatenate([(r16[0] - r64[0]).ravel(), (r16[1] - r64[1]).ravel()]), expec_f=r16[2] - r64[2],
                    mkpts1_f=r16[3] - r64[3])
        for k, e in errs.items():
            rec[f"{case}_{k}_e16_rms"], rec[f"{case}_{k}_e16_max"] = np.float64(rms(e)), np.float64(np.abs(e).max())
            print(f"  {k}: e16_rms {rms(e):.3e}  e16_max {np.abs(e).max():.3e}")
        rec[f"{case}_xy_rms"], rec[f"{case}_xy_e16_max"] = np.float64(xy_rms), np.float64(xy_e16)
        print(f"  win rms {rms(np.concatenate([r64[0].ravel(), r64[1].ravel()])):.3f}  std column mean {r64[2][:, 2].mean():.3f}")

    # No committed file may pass 1 MiB: the arrays are cut along their first axis ("key@n") and dealt to
    # shards fine_match.npz, fine_match.1.npz, ... by their compressed size (the inputs hold fp16 values and
    # compress well, the float64 outputs do not); fine_oracle.load_golden puts them together again.
    parts = {}
    for k, v in rec.items():
        v = np.asarray(v)
        if v.ndim >= 2 and v.nbytes > 100_000:
            parts.update({f"{k}@{n}": v[n:n + 1] for n in range(v.shape[0])})
        else:
            parts[k] = v
    shards, room = [{}], O.SHARD_BYTES
    for k, v in parts.items():
        size = len(zlib.compress(np.ascontiguousarray(v).tobytes(), 6)) + 256
        if size > room and shards[-1]:
            shards.append({})
            room = O.SHARD_BYTES
        shards[-1][k] = v
        room -= size
    shards[0]["n_shards"] = np.array(len(shards))
    for n, sh in enumerate(shards):
        out = os.path.join(HERE, O.shard_name(n))
        np.savez_compressed(out, **sh)
        print(out, os.path.getsize(out), "bytes")
        assert os.path.getsize(out) < 1 << 20


if __name__ == "__main__":
    main()
