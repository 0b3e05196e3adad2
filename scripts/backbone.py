"""Time the backbone at the reference's shapes and record the figures and the parity.

10 frames of 400 x 400 (a window of cropped frames) and 15 of 640 x 480, seeded uniform images and the
weights of tests/backbone_oracle.py, against the same network written with torch ops (conv2d, batch_norm,
interpolate) under fp16 autocast on the same GPU. Per shape: host clock around the whole call (input
conversion, validation, twenty launches) to a device synchronise, median of 3 after a warm-up; the peak
allocation of a call; and the achieved fraction of the dense fp16 MFMA peak, the network's arithmetic computed
from the layer shapes over the call's time. Kernel time alone is not measured. Written to
profiles/r22/backbone.json, not asserted.

The parity of the three cases of tests/backbone_oracle.py against tests/golden/backbone*.npz (error over
the reference's own fp16-autocast error e16) goes to profiles/r22/parity_backbone.json.

    python scripts/backbone.py [--out-dir profiles/r22]
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

from scripts.transformer import _median_ms, _peak  # noqa: E402

PEAK_FP16 = 2.5e15          # dense fp16 MFMA, FLOP/s


def flops(H, W):
    """Multiply-adds times two of one image, from the layer shapes (channels as the reference counts them)."""
    from tests import backbone_oracle as O
    level = {"conv1": 2, "layer1": 2, "layer2": 4, "layer3": 8, "layer3_outconv": 8, "layer2_outconv": 4,
             "layer2_outconv2": 4, "layer1_outconv": 2, "layer1_outconv2": 2}
    total = 0
    for name, (cout, cin, k) in O.conv_shapes().items():
        s = level[name.split(".")[0]]
        total += 2 * cout * cin * k * k * (H // s) * (W // s)
    return total


def torch_backbone(w, x):
    """ResNetFPN_8_2 in eval mode with torch ops: x [N,1,H,W] -> (coarse [N,256,H/8,W/8], fine [N,128,H/2,W/2])."""
    conv = lambda v, name, stride=1: F.conv2d(v, w[name + ".weight"], stride=stride, padding=w[name + ".weight"].shape[-1] // 2)
    bn = lambda v, name: F.batch_norm(v, w[name + ".running_mean"], w[name + ".running_var"], w[name + ".weight"],
                                      w[name + ".bias"], False, 0.0, 1e-5)

    def block(v, p, stride):
        y = F.relu(bn(conv(v, p + ".conv1", stride), p + ".bn1"))
        y = bn(conv(y, p + ".conv2"), p + ".bn2")
        if stride != 1:
            v = bn(conv(v, p + ".downsample.0", stride), p + ".downsample.1")
        return F.relu(v + y)

    def head(v, p):
        return conv(F.leaky_relu(bn(conv(v, p + ".0"), p + ".1")), p + ".3")

    with torch.autocast("cuda", dtype=torch.float16):
        x0 = F.relu(bn(conv(x, "conv1", 2), "bn1"))
        x1 = block(block(x0, "layer1.0", 1), "layer1.1", 1)
        x2 = block(block(x1, "layer2.0", 2), "layer2.1", 1)
        x3 = block(block(x2, "layer3.0", 2), "layer3.1", 1)
        x3_out = conv(x3, "layer3_outconv")
        up = lambda v: F.interpolate(v, scale_factor=2.0, mode="bilinear", align_corners=True)
        x2_out = head(conv(x2, "layer2_outconv") + up(x3_out), "layer2_outconv2")
        x1_out = head(conv(x1, "layer1_outconv") + up(x2_out), "layer1_outconv2")
    return x3_out, x1_out


def time_shape(dev, net, wt, N, H, W, seed=22):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.rand((N, H, W), generator=gen).half().float().to(dev)
    fused = lambda: net.forward(x)
    route = lambda: torch_backbone(wt, x[:, None])
    res = dict(frames=N, image=[H, W], flop=N * flops(H, W))
    res["fused_ms"], res["fused_ms_all"] = _median_ms(fused)
    res["torch_autocast_ms"], res["torch_autocast_ms_all"] = _median_ms(route)
    res["fused_peak_bytes_allocated"] = _peak(fused)
    res["torch_peak_bytes_allocated"] = _peak(route)
    res["scratch_bytes"] = int(net._scratch[x.device].numel())
    res["fused_fraction_of_fp16_mfma_peak"] = res["flop"] / (1e-3 * res["fused_ms"]) / PEAK_FP16
    res["torch_fraction_of_fp16_mfma_peak"] = res["flop"] / (1e-3 * res["torch_autocast_ms"]) / PEAK_FP16
    tok, fine, (hc, wc) = net.forward(x, position_encoding=False)
    c2, f2 = route()
    dc = tok.view(N, hc, wc, 256).permute(0, 3, 1, 2) - c2.float()
    df = fine.permute(0, 3, 1, 2).float() - f2.float()
    res["coarse_rms"], res["fine_rms"] = float(c2.float().square().mean().sqrt()), float(f2.float().square().mean().sqrt())
    res["coarse_rms_difference_of_the_two_routes"] = float(dc.square().mean().sqrt())
    res["fine_rms_difference_of_the_two_routes"] = float(df.square().mean().sqrt())
    res["finite"] = bool(torch.isfinite(tok).all() and torch.isfinite(fine).all())
    return res


def parity(dev, net):
    from tests import backbone_oracle as O
    g = O.load_golden(os.path.join(ROOT, "tests", "golden"))
    rows = {}
    for case, c in O.CASES.items():
        tok, fine, (hc, wc) = net.forward(O.make_images(case), position_encoding=False)
        got = dict(coarse=tok.double().cpu().numpy().reshape(c["N"], hc, wc, 256).transpose(0, 3, 1, 2),
                   fine=fine.double().cpu().numpy().transpose(0, 3, 1, 2))
        for k, v in got.items():
            e = v - g[f"{case}_{k}64"]
            rms, mx = float(np.sqrt(np.mean(e ** 2))), float(np.abs(e).max())
            e_rms, e_max = float(g[f"{case}_{k}_e16_rms"]), float(g[f"{case}_{k}_e16_max"])
            rows[f"{case}/{k}"] = dict(rms=rms, max=mx, e16_rms=e_rms, e16_max=e_max, rms_over_e16=rms / e_rms,
                                       max_over_e16=mx / e_max)
    return rows


def main():
    from bundlesdf_amd.backbone import Backbone
    from tests import backbone_oracle as O
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "r22"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    os.makedirs(args.out_dir, exist_ok=True)
    w = O.make_weights()
    net = Backbone(w, device=dev)
    par = dict(device=torch.cuda.get_device_name(0), bound="2 x e16 (tests/test_gpu_backbone.py)", cases=parity(dev, net))
    with open(os.path.join(args.out_dir, "parity_backbone.json"), "w") as f:
        json.dump(par, f, indent=1)
    wt = {k: torch.from_numpy(v).to(dev) for k, v in w.items()}
    res = dict(device=torch.cuda.get_device_name(0),
               timing="host clock around each call (input conversion, validation, launches) to a device synchronise, "
                      "median of 3 after a warm-up; kernel time alone and the layers apart not measured",
               fp16_mfma_peak_flops=PEAK_FP16,
               crops=time_shape(dev, net, wt, 10, 400, 400), frames=time_shape(dev, net, wt, 15, 480, 640))
    with open(os.path.join(args.out_dir, "backbone.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(parity={k: (round(v["rms_over_e16"], 3), round(v["max_over_e16"], 3)) for k, v in par["cases"].items()},
                          ms={k: (res[k]["fused_ms"], res[k]["torch_autocast_ms"]) for k in ("crops", "frames")})))


if __name__ == "__main__":
    main()
