"""Time the feature transformer at the reference's shapes and record the figures and the parity.

Coarse: 45 pairs x 2500 + 2500 tokens x 256 channels x 8 layers (the 1/8 grid of a 400-pixel image,
every pair of a 10-frame window). Fine: 20000 windows x 25 + 25 tokens x 128 channels x 2 layers.
FeatureTransformer.forward against the same stack written with torch ops on the same GPU under fp16
autocast (torch_stack below). Medians of 3 calls after one warm-up, a host clock around the whole call
(conversion of the inputs, validation, launches) ending in a device synchronise; kernel time alone is
not measured. Peak allocated memory is taken for both routes. The figures are recorded in
profiles/r20/transformer.json, not asserted.

The parity of the six cases of tests/transformer_oracle.py against tests/golden/feature_transformer*.npz
(error over the reference's own half-precision error, the bound of tests/test_gpu_transformer.py being
2) goes to profiles/r20/parity_transformer.json.

    python scripts/transformer.py [--out-dir profiles/r20] [--pairs 45] [--tokens 2500] [--windows 20000]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

H = 8


def torch_layer(w, i, x, src):
    """One application with torch ops (meant to run under autocast): [P,L,C], [P,S,C] -> [P,L,C]."""
    g = lambda name: w[f"layers.{i}.{name}"]
    P, L, C = x.shape
    S, D = src.shape[1], C // H
    q = (F.elu(F.linear(x, g("q_proj.weight"))) + 1).view(P, L, H, D)
    k = (F.elu(F.linear(src, g("k_proj.weight"))) + 1).view(P, S, H, D)
    v = F.linear(src, g("v_proj.weight")).view(P, S, H, D) / S
    kv = torch.einsum("pshd,pshe->phde", k, v)
    z = 1 / (torch.einsum("plhd,phd->plh", q, k.sum(1)) + 1e-6)
    msg = (torch.einsum("plhd,phde,plh->plhe", q, kv, z) * S).reshape(P, L, C)
    m = F.layer_norm(F.linear(msg, g("merge.weight")), (C,), g("norm1.weight"), g("norm1.bias"))
    m = F.linear(F.relu(F.linear(torch.cat([x, m], 2), g("mlp.0.weight"))), g("mlp.2.weight"))
    return x + F.layer_norm(m, (C,), g("norm2.weight"), g("norm2.bias"))


def torch_stack(w, names, a, b):
    with torch.autocast("cuda", dtype=torch.float16):
        for i, n in enumerate(names):
            if n == "self":
                a, b = torch_layer(w, i, a, a), torch_layer(w, i, b, b)
            else:
                a = torch_layer(w, i, a, b)
                b = torch_layer(w, i, b, a)
    return a, b


def _median_ms(call, reps=3):
    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t))
    return float(np.median(ts)), ts


def _peak(call):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = call()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def time_shape(T, O, dev, P, L, S, C, names, seed, check_pairs):
    w = O.make_weights(seed, C, names)
    ft = T.FeatureTransformer(w, d_model=C, layer_names=names, device=dev)
    wt = {k: torch.from_numpy(v).to(dev) for k, v in w.items()}
    gen = torch.Generator(device="cpu").manual_seed(seed)
    a = torch.randn((P, L, C), generator=gen).half().float().to(dev)
    b = torch.randn((P, S, C), generator=gen).half().float().to(dev)
    res = dict(P=P, L=L, S=S, C=C, layers=list(names))
    res["flop"] = 20 * C * C * (L + S) * P * len(names)          # 20 C^2 per token and layer, arithmetic not a timing
    res["fused_ms"], res["fused_ms_all"] = _median_ms(lambda: ft.forward(a, b))
    res["torch_autocast_ms"], res["torch_autocast_ms_all"] = _median_ms(lambda: torch_stack(wt, names, a, b))
    res["fused_peak_bytes_allocated"] = _peak(lambda: ft.forward(a, b))      # outputs and, on a first call, the workspace
    res["torch_peak_bytes_allocated"] = _peak(lambda: torch_stack(wt, names, a, b))
    res["workspace_bytes"] = int(ft._workspace[a.device].numel())
    res["packed_weight_bytes"] = int(ft.packed.size)
    oa, ob = ft.forward(a, b)
    ra, rb = torch_stack(wt, names, a, b)
    d = torch.cat([(oa - ra.float()).flatten(), (ob - rb.float()).flatten()])
    res["rms_difference_of_the_two_routes"] = float(d.square().mean().sqrt())
    res["max_difference_of_the_two_routes"] = float(d.abs().max())
    res["finite"] = bool(torch.isfinite(oa).all() and torch.isfinite(ob).all())
    # both routes against the float64 oracle (numpy, on the host) on the first pairs: at long sequences the
    # autocast route holds Z = Q . Ksum in fp16, which can pass 65504
    n = min(P, check_pairs)
    wa, wb = O.forward(w, names, a[:n].cpu().numpy(), b[:n].cpu().numpy())
    for label, xa, xb in (("fused", oa, ob), ("torch_autocast", ra, rb)):
        e = np.concatenate([(xa[:n].double().cpu().numpy() - wa).ravel(), (xb[:n].double().cpu().numpy() - wb).ravel()])
        res[f"{label}_vs_float64_oracle"] = dict(pairs=n, rms=float(np.sqrt(np.mean(e ** 2))), max=float(np.abs(e).max()),
                                                 finite=bool(np.isfinite(e).all()))
    res["oracle_output_rms"] = float(np.sqrt(np.mean(np.concatenate([wa.ravel(), wb.ravel()]) ** 2)))
    return res


def parity(T, O, dev):
    g = O.load_golden(os.path.join(ROOT, "tests", "golden"))
    rows = {}
    for case, c in O.CASES.items():
        w, a, b, ma, mb = O.case_data(case)
        ft = T.FeatureTransformer(w, d_model=c["C"], layer_names=c["layers"], device=dev)
        runs = [("plain", None, None, "64")] + ([("masked", ma, mb, "64m")] if ma is not None else [])
        for label, xa, xb, key in runs:
            oa, ob = ft.forward(a, b, xa, xb)
            err = np.concatenate([(oa.double().cpu().numpy() - g[f"{case}_a{key}"]).ravel(),
                                  (ob.double().cpu().numpy() - g[f"{case}_b{key}"]).ravel()])
            rms, mx = float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())
            rows[f"{case}/{label}"] = dict(rms=rms, max=mx, e16_rms=float(g[f"{case}_e16_rms"]),
                                           e16_max=float(g[f"{case}_e16_max"]), rms_over_e16=rms / float(g[f"{case}_e16_rms"]),
                                           max_over_e16=mx / float(g[f"{case}_e16_max"]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r20"))
    ap.add_argument("--pairs", type=int, default=45)
    ap.add_argument("--tokens", type=int, default=2500)
    ap.add_argument("--windows", type=int, default=20000)
    args = ap.parse_args()
    from bundlesdf_amd import transformer as T
    from tests import transformer_oracle as O

    dev = torch.device("cuda", 0)
    os.makedirs(args.out_dir, exist_ok=True)
    par = dict(device=torch.cuda.get_device_name(0), bound="2 x e16 (tests/test_gpu_transformer.py)", cases=parity(T, O, dev))
    with open(os.path.join(args.out_dir, "parity_transformer.json"), "w") as f:
        json.dump(par, f, indent=1)
    res = dict(device=torch.cuda.get_device_name(0),
               timing="host clock around each call (input copies, validation, launches) to a device synchronise, median "
                      "of 3 after a warm-up; kernel time alone not measured",
               coarse=time_shape(T, O, dev, args.pairs, args.tokens, args.tokens, 256, ("self", "cross") * 4, 11, 1),
               fine=time_shape(T, O, dev, args.windows, 25, 25, 128, ("self", "cross"), 12, 8))
    with open(os.path.join(args.out_dir, "transformer.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(parity={k: (round(v["rms_over_e16"], 3), round(v["max_over_e16"], 3)) for k, v in par["cases"].items()},
                          coarse_ms=(res["coarse"]["fused_ms"], res["coarse"]["torch_autocast_ms"]),
                          fine_ms=(res["fine"]["fused_ms"], res["fine"]["torch_autocast_ms"]))))


if __name__ == "__main__":
    main()
