"""Time the fine-level refinement at the reference's shape and record the figures and the parity.

20000 matches over the 45 pairs of a 10-frame window, fine maps 200 x 200 x 128, coarse grids 50 x 50 x 256
(the 1/2 and 1/8 grids of a 400-pixel image): the shape scripts/transformer.py calls fine.
FineRefiner.refine against the same stage written with torch ops on the same GPU under fp16 autocast
(torch_refine below: F.unfold of every cell of the maps the pairs use, the index, the two Linears, the
torch transformer of scripts/transformer.py, einsum, softmax and the moments). Medians of 3 calls after
one warm-up, a host clock around the whole call (conversion of the maps, validation, the one host read,
launches) ending in a device synchronise; kernel time alone and the three stages apart are not measured.
refine is timed with channels-first float32 maps (converted inside the call) and with channels-last fp16
maps (used as they are). Peak allocated memory is taken for both routes. The figures are recorded in
profiles/r21/fine.json, not asserted.

The parity of the two cases of tests/fine_oracle.py against tests/golden/fine_match*.npz (error over the
reference's own half-precision error, the bound of tests/test_gpu_fine.py being 2) goes to
profiles/r21/parity_fine.json.

    python scripts/fine.py [--out-dir profiles/r21] [--matches 20000] [--frames 10] [--grid 50]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from scripts.transformer import _median_ms, _peak, torch_stack  # noqa: E402


def torch_refine(wt, names, pair, i, j, fine_a, fine_b, frames_a, frames_b, coarse_a, coarse_b, stride):
    """The reference's three stages with torch ops: fine_* [N,128,hf,wf], coarse_* [P,n,256] -> expec [M,3]."""
    g = lambda k: wt["fine_preprocess." + k]
    with torch.autocast("cuda", dtype=torch.float16):
        def unfold(f):
            u = F.unfold(f, kernel_size=(5, 5), stride=stride, padding=2)              # [N, 128 25, L]
            return u.view(f.shape[0], 128, 25, -1).permute(0, 3, 2, 1)                  # 'n (c ww) l -> n l ww c'
        ua, ub = unfold(fine_a)[frames_a[pair], i], unfold(fine_b)[frames_b[pair], j]   # [M,25,128]
        ctx = F.linear(torch.cat([coarse_a[pair, i], coarse_b[pair, j]], 0), g("down_proj.weight"), g("down_proj.bias"))
        both = torch.cat([torch.cat([ua, ub], 0), ctx[:, None].expand(-1, 25, -1)], -1)
        wa, wb = torch.chunk(F.linear(both, g("merge_feat.weight"), g("merge_feat.bias")), 2, dim=0)
        w_ft = {k[len("loftr_fine."):]: v for k, v in wt.items() if k.startswith("loftr_fine.")}
    f0, f1 = torch_stack(w_ft, names, wa, wb)
    with torch.autocast("cuda", dtype=torch.float16):
        sim = torch.einsum("mc,mrc->mr", f0[:, 12], f1)
        heat = torch.softmax(sim / 128 ** 0.5, dim=1)
        r = torch.arange(25, device=heat.device)
        grid = torch.stack([-1 + 0.5 * (r % 5), -1 + 0.5 * (r // 5)], 1).float()
        mean = heat @ grid
        var = heat @ grid ** 2 - mean ** 2
        std = torch.sqrt(torch.clamp(var, min=1e-10)).sum(-1)
    return torch.cat([mean, std[:, None]], -1)


def time_shape(dev, n_matches, n_frames, grid, seed=21):
    from bundlesdf_amd.fine import FineRefiner
    from bundlesdf_amd.matching import CoarseMatches
    from tests import fine_oracle as O
    stride, L = 4, grid * grid
    pairs = np.array([(a, b) for a in range(n_frames) for b in range(a + 1, n_frames)])
    P = len(pairs)
    rng = np.random.default_rng(seed)
    per = [n_matches // P + (1 if p < n_matches % P else 0) for p in range(P)]
    j_of_i = np.full((P, L), -1, np.int32)
    for p, n in enumerate(per):
        j_of_i[p, rng.choice(L, n, replace=False)] = rng.choice(L, n, replace=False)
    conf = np.where(j_of_i >= 0, 0.5, 0.0).astype(np.float32)
    cm = CoarseMatches(j_of_i=torch.from_numpy(j_of_i).to(dev), conf=torch.from_numpy(conf).to(dev),
                       n_matches=torch.from_numpy(np.array(per, np.int32)).to(dev), hw_a=(grid, grid), hw_b=(grid, grid))
    w = O.make_weights(seed)
    refiner = FineRefiner(w, device=dev)
    wt = {k: torch.from_numpy(v).to(dev) for k, v in w.items()}
    gen = torch.Generator(device="cpu").manual_seed(seed)
    fine = torch.randn((n_frames, 128, stride * grid, stride * grid), generator=gen).half().float().to(dev)
    fine_cl = fine.permute(0, 2, 3, 1).half().contiguous()
    ca = torch.randn((P, L, 256), generator=gen).half().float().to(dev)
    cb = torch.randn((P, L, 256), generator=gen).half().float().to(dev)
    fr_a, fr_b = torch.from_numpy(pairs[:, 0]).to(dev), torch.from_numpy(pairs[:, 1]).to(dev)
    pair_t, i_t = torch.nonzero(cm.j_of_i >= 0, as_tuple=True)
    j_t = cm.j_of_i[pair_t, i_t].long()

    fused = lambda: refiner.refine(cm, fine, fine, ca, cb, frames_a=fr_a, frames_b=fr_b).expec
    fused_cl = lambda: refiner.refine(cm, fine_cl, fine_cl, ca, cb, frames_a=fr_a, frames_b=fr_b).expec
    route = lambda: torch_refine(wt, O.LAYERS, pair_t, i_t, j_t, fine, fine, fr_a, fr_b, ca, cb, stride)
    res = dict(matches=int(n_matches), pairs=P, frames=n_frames, fine_map=[stride * grid, stride * grid], coarse_grid=[grid, grid],
               chunk=8192)
    res["fused_ms"], res["fused_ms_all"] = _median_ms(fused)
    res["fused_channels_last_fp16_ms"], res["fused_channels_last_fp16_ms_all"] = _median_ms(fused_cl)
    res["torch_autocast_ms"], res["torch_autocast_ms_all"] = _median_ms(route)
    res["fused_peak_bytes_allocated"] = _peak(fused)
    res["fused_channels_last_fp16_peak_bytes_allocated"] = _peak(fused_cl)
    res["torch_peak_bytes_allocated"] = _peak(route)
    res["transformer_workspace_bytes"] = int(refiner.transformer._workspace[ca.device].numel())
    a, b = fused(), route().float()
    assert torch.equal(a, fused_cl())
    d = a - b
    res["rms_difference_of_the_two_routes"] = float(d.square().mean().sqrt())
    res["max_difference_of_the_two_routes"] = float(d.abs().max())
    res["xy_rms"] = float(a[:, :2].square().mean().sqrt())
    res["finite"] = bool(torch.isfinite(a).all())
    return res


def parity(dev):
    from bundlesdf_amd.fine import FineRefiner
    from bundlesdf_amd.matching import CoarseMatches
    from tests import fine_oracle as O
    g = O.load_golden(os.path.join(ROOT, "tests", "golden"))
    rows = {}
    for case, c in O.CASES.items():
        r = FineRefiner(O.make_weights(c["seed"]), device=dev)
        fa, fb, ca, cb = (torch.from_numpy(g[f"{case}_{k}"]).float().to(dev) for k in ("fine_a", "fine_b", "coarse_a", "coarse_b"))
        pair, i, j, j_of_i = O.case_matches(case)
        cm = CoarseMatches(j_of_i=torch.from_numpy(j_of_i).to(dev), conf=torch.from_numpy((j_of_i >= 0).astype(np.float32)).to(dev),
                           n_matches=None, hw_a=c["hw_a"], hw_b=c["hw_b"])
        fm = r.refine(cm, fa, fb, ca, cb, frames_a=c["frames_a"], frames_b=c["frames_b"])
        cl = lambda t: t.permute(0, 2, 3, 1).half().contiguous()
        wa, wb = r.windows(pair, i, j, cl(fa), cl(fb), ca, cb, c["hw_a"], c["hw_b"], c["frames_a"], c["frames_b"])
        errs = dict(win=np.concatenate([(wa.double().cpu().numpy() - g[f"{case}_win_a"]).ravel(),
                                        (wb.double().cpu().numpy() - g[f"{case}_win_b"]).ravel()]),
                    expec_f=fm.expec.double().cpu().numpy() - g[f"{case}_expec_f"],
                    mkpts1_f=fm.to_pixels(scale=c["stride"] * O.SCALE_F, rounded=False)[1].cpu().numpy() - g[f"{case}_mkpts1_f"])
        for k, e in errs.items():
            rms, mx = float(np.sqrt(np.mean(e ** 2))), float(np.abs(e).max())
            e_rms, e_max = float(g[f"{case}_{k}_e16_rms"]), float(g[f"{case}_{k}_e16_max"])
            rows[f"{case}/{k}"] = dict(rms=rms, max=mx, e16_rms=e_rms, e16_max=e_max, rms_over_e16=rms / e_rms,
                                       max_over_e16=mx / e_max)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r21"))
    ap.add_argument("--matches", type=int, default=20000)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--grid", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    os.makedirs(args.out_dir, exist_ok=True)
    par = dict(device=torch.cuda.get_device_name(0), bound="2 x e16 (tests/test_gpu_fine.py)", cases=parity(dev))
    with open(os.path.join(args.out_dir, "parity_fine.json"), "w") as f:
        json.dump(par, f, indent=1)
    res = dict(device=torch.cuda.get_device_name(0),
               timing="host clock around each call (map conversion, validation, one host read, launches) to a device "
                      "synchronise, median of 3 after a warm-up; kernel time alone and the stages apart not measured",
               fine=time_shape(dev, args.matches, args.frames, args.grid))
    with open(os.path.join(args.out_dir, "fine.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(parity={k: (round(v["rms_over_e16"], 3), round(v["max_over_e16"], 3)) for k, v in par["cases"].items()},
                          fine_ms=(res["fine"]["fused_ms"], res["fine"]["fused_channels_last_fp16_ms"],
                                   res["fine"]["torch_autocast_ms"]))))


if __name__ == "__main__":
    main()
