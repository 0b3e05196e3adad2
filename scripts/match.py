"""Time descriptor matching at the reference's shapes and record the figures.

45 pairs x 2500 x 2500 cells x 256 channels (the 1/8 grid of a 400-pixel image, every pair of a 10-frame
window): match_descriptors against the materialised torch route on the same GPU, which is what the
reference's matching head does in autocast: an fp16 einsum, two softmaxes, their product, two max
passes and the comparisons, each [45,2500,2500] array written to and read from HBM. Medians of 3 calls
after one warm-up, a host clock around the whole call ending in a device synchronise; kernel time
alone is not measured. The figures are recorded in profiles/r19/match.json, not asserted.

    python scripts/match.py [--out profiles/r19/match.json] [--pairs 45] [--cells 50]
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


def materialised(a, b, hw, temperature=0.1, thr=0.2, border_rm=2):
    """The reference's route in torch on the device: fp16 einsum, float32 from the softmaxes on."""
    C = a.shape[-1]
    sim = torch.einsum("nlc,nsc->nls", a / C ** .5, b / C ** .5).float() / temperature
    conf = torch.softmax(sim, 1) * torch.softmax(sim, 2)
    mask = conf > thr
    P, (h, w) = conf.shape[0], hw
    m5 = mask.view(P, h, w, h, w)
    if border_rm > 0:
        bd = border_rm
        m5[:, :bd] = False
        m5[:, :, :bd] = False
        m5[:, :, :, :bd] = False
        m5[:, :, :, :, :bd] = False
        m5[:, -bd:] = False
        m5[:, :, -bd:] = False
        m5[:, :, :, -bd:] = False
        m5[:, :, :, :, -bd:] = False
    mask = mask & (conf == conf.max(dim=2, keepdim=True)[0]) & (conf == conf.max(dim=1, keepdim=True)[0])
    mask_v, all_j = mask.max(dim=2)
    return torch.where(mask_v, all_j, -1), mask_v.sum(1)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "match.json"))
    ap.add_argument("--pairs", type=int, default=45)
    ap.add_argument("--cells", type=int, default=50)
    ap.add_argument("--channels", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("match.py times the device path: no HIP device")
    from bundlesdf_amd.matching import match_descriptors
    from bundlesdf_amd import _lib
    dev = torch.device("cuda", 0)
    P, n, C = args.pairs, args.cells, args.channels
    L = n * n
    g = torch.Generator(device="cpu").manual_seed(0)
    a = (1.4 * torch.randn(P, L, C, generator=g)).half()
    b = (1.4 * torch.randn(P, L, C, generator=g)).half()
    for p in range(P):                                     # two thirds of B's rows copy rows of A, with 5 % noise
        src, dst = torch.randperm(L, generator=g)[:2 * L // 3], torch.randperm(L, generator=g)[:2 * L // 3]
        b[p, dst] = (a[p, src].float() * (1.0 + 0.05 * torch.randn(len(src), C, generator=g))).half()
    a, b = a.to(dev), b.to(dev)
    hw = (n, n)
    got = match_descriptors(a, b, hw, hw)
    want_j, want_n = materialised(a, b, hw)
    torch.cuda.synchronize()
    fused_ms, fused_all = _median_ms(lambda: match_descriptors(a, b, hw, hw))
    torch.cuda.empty_cache()
    mat_ms, mat_all = _median_ms(lambda: materialised(a, b, hw))
    peak = torch.cuda.max_memory_allocated(dev)
    res = dict(pairs=P, L=L, S=L, C=C, device=torch.cuda.get_device_name(0),
               timing="host clock around each call (validation, launches) to a device synchronise, median of 3 after a "
                      "warm-up; kernel time alone not measured",
               match_descriptors_ms=fused_ms, match_descriptors_ms_all=fused_all,
               materialised_torch_ms=mat_ms, materialised_torch_ms_all=mat_all,
               workspace_bytes=int(_lib.lib().nof_match_workspace_bytes(P, L, L)), one_LS_array_bytes=P * L * L * 4,
               torch_peak_bytes_allocated=int(peak),
               gemm_flop_per_pass=2 * P * L * L * C, gemm_passes=4,
               matches=int(got.n_matches.sum().item()), materialised_matches=int(want_n.sum().item()),
               rows_with_another_partner=int((got.j_of_i != want_j).sum().item()),
               note="the materialised route sums in another order and keeps fp16 sim; rows that differ are counted, "
                    "not asserted")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
