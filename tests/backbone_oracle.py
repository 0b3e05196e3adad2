"""Float64 numpy restatement of the backbone's definition (the header comment of
bundlesdf_amd/csrc/backbone.hip), with the generators of the weights and inputs the tests and
tests/golden/make_backbone.py share. Nothing here is stored: weights and inputs are drawn again from
their seeds wherever they are needed.

    x0 = relu(bn1(conv7x7 s2 p3 (1 -> 128)))                               1/2
    layer1 = BasicBlock(128,128), BasicBlock(128,128)                      1/2   -> x1
    layer2 = BasicBlock(128,196, s2), BasicBlock(196,196)                  1/4   -> x2
    layer3 = BasicBlock(196,256, s2), BasicBlock(256,256)                  1/8   -> x3
    x3_out = conv1x1(x3);  x2_out = outconv2(conv1x1(x2) + up2(x3_out));  x1_out = outconv2(conv1x1(x1) + up2(x2_out))

forward(..., rounded=False) is the network as the reference states it, BatchNorm applied after each
convolution. rounded=True puts the device's fp16 rounding points in: the image, the folded weights
(W' = W g / sqrt(var + eps), once), every stored activation, the fp16 copy of x3_out that up2 reads; b' and
the up2 coordinates are float32, the fused skip of a down-sampling block is not rounded on its own, and the
coarse output is not rounded.
"""
import os

import numpy as np

EPS = 1e-5
LRELU = 0.01
SEED = 2201

# name -> N, H, W, seed of the input
CASES = {
    "one_cell": dict(N=1, H=8, W=8, seed=301),
    "ragged": dict(N=2, H=40, W=56, seed=302),
    "wide": dict(N=1, H=24, W=72, seed=303),
}
SHARD_BYTES = 900_000                           # array bytes per fixture shard (float64 does not compress)

_BLOCKS = {1: (128, 128), 2: (128, 196), 3: (196, 256)}      # stage -> (Cin, C)


def conv_shapes():
    """The reference's convolution names -> (Cout, Cin, KH), in the order of its state dict."""
    s = {"conv1": (128, 1, 7)}
    for st, (cin, c) in _BLOCKS.items():
        s[f"layer{st}.0.conv1"] = (c, cin, 3)
        s[f"layer{st}.0.conv2"] = (c, c, 3)
        if st > 1:
            s[f"layer{st}.0.downsample.0"] = (c, cin, 1)
        s[f"layer{st}.1.conv1"] = (c, c, 3)
        s[f"layer{st}.1.conv2"] = (c, c, 3)
    s.update({"layer3_outconv": (256, 256, 1), "layer2_outconv": (256, 196, 1), "layer2_outconv2.0": (256, 256, 3),
              "layer2_outconv2.3": (196, 256, 3), "layer1_outconv": (196, 128, 1), "layer1_outconv2.0": (196, 196, 3),
              "layer1_outconv2.3": (128, 196, 3)})
    return s


def norm_shapes():
    """The reference's BatchNorm names -> channels."""
    s = {"bn1": 128}
    for st, (_, c) in _BLOCKS.items():
        for b in (0, 1):
            s[f"layer{st}.{b}.bn1"] = s[f"layer{st}.{b}.bn2"] = c
        if st > 1:
            s[f"layer{st}.0.downsample.1"] = c
    s.update({"layer2_outconv2.1": 256, "layer1_outconv2.1": 196})
    return s


def make_weights(seed=SEED):
    """The reference's parameter names -> float32 arrays. Convolutions N(0, 2 / fan_in) (kaiming); BatchNorm
    weight in 0.75 .. 1.25, bias and running_mean 0.2 N(0,1), running_var in 0.5 .. 1.5, so that a wrong fold
    shows."""
    rng = np.random.default_rng(seed)
    w = {}
    for name, (cout, cin, k) in conv_shapes().items():
        w[name + ".weight"] = (rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
    for name, c in norm_shapes().items():
        w[name + ".weight"] = rng.uniform(0.75, 1.25, c).astype(np.float32)
        w[name + ".bias"] = (0.2 * rng.standard_normal(c)).astype(np.float32)
        w[name + ".running_mean"] = (0.2 * rng.standard_normal(c)).astype(np.float32)
        w[name + ".running_var"] = rng.uniform(0.5, 1.5, c).astype(np.float32)
    return w


def make_images(case):
    """[N,H,W] uniform [0,1), float32 arrays of fp16 values."""
    c = CASES[case]
    rng = np.random.default_rng(c["seed"])
    return rng.random((c["N"], c["H"], c["W"])).astype(np.float16).astype(np.float32)


def case_data(case):
    """(weights, images) of a case."""
    return make_weights(), make_images(case)


def shard_name(i):
    return "backbone.npz" if i == 0 else f"backbone.{i}.npz"


def load_golden(golden_dir):
    """tests/golden/backbone*.npz as one dict; the per-image parts "key@n" stacked on a leading axis."""
    first = np.load(os.path.join(golden_dir, shard_name(0)))
    flat = {}
    for i in range(int(first["n_shards"])):
        with np.load(os.path.join(golden_dir, shard_name(i))) as z:
            flat.update({k: z[k] for k in z.files})
    out, parts = {}, {}
    for k, v in flat.items():
        if "@" in k:
            key, n = k.split("@")
            parts.setdefault(key, {})[int(n)] = v
        else:
            out[k] = v
    for key, d in parts.items():
        out[key] = np.stack([d[n] for n in range(len(d))])
    return out


def _f16(x):
    return x.astype(np.float16).astype(np.float64)


def conv(x, W, stride):
    """x [N,H,W,Cin] f64, W [Cout,Cin,K,K], zero padding K // 2 -> [N,Ho,Wo,Cout] f64."""
    cout, cin, k, _ = W.shape
    pad = k // 2
    N, H, Wd, _ = x.shape
    ho, wo = (H + 2 * pad - k) // stride + 1, (Wd + 2 * pad - k) // stride + 1
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    cols = np.concatenate([xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride, :]
                           for ky in range(k) for kx in range(k)], axis=3)
    return cols @ W.astype(np.float64).transpose(0, 2, 3, 1).reshape(cout, k * k * cin).T


def fold(w, conv_name, bn_name):
    """(W' f64 of fp16 values, b' f64 of f32 values) of a convolution and the BatchNorm after it."""
    W = w[conv_name + ".weight"].astype(np.float64)
    if bn_name is None:
        return _f16(W), np.zeros(W.shape[0])
    g, b, m, v = (w[f"{bn_name}.{k}"].astype(np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
    s = g / np.sqrt(v + EPS)
    return _f16(W * s[:, None, None, None]), (b - m * s).astype(np.float32).astype(np.float64)


def up2(x, rounded):
    """x [N,h,w,C] -> [N,2h,2w,C], bilinear, align_corners=True, in the order the definition states."""
    ft = np.float32 if rounded else np.float64

    def coords(h):
        y = np.arange(2 * h)
        s = (y * (h - 1)).astype(ft) / ft(2 * h - 1)
        y0 = np.floor(s).astype(np.int64)
        return y0, np.minimum(y0 + 1, h - 1), (s - y0.astype(ft)).astype(ft)

    _, h, w, _ = x.shape
    y0, y1, fy = coords(h)
    x0, x1, fx = coords(w)
    x = x.astype(ft)
    fy, fx = fy[None, :, None, None], fx[None, None, :, None]
    top = (1 - fx) * x[:, y0][:, :, x0] + fx * x[:, y0][:, :, x1]
    bot = (1 - fx) * x[:, y1][:, :, x0] + fx * x[:, y1][:, :, x1]
    return ((1 - fy) * top + fy * bot).astype(np.float64)


def forward(w, images, rounded=False):
    """images [N,H,W] -> (coarse [N,256,H/8,W/8], fine [N,128,H/2,W/2]) float64, the module's layout."""
    r = _f16 if rounded else (lambda v: v)

    def cb(x, conv_name, bn_name, stride=1):
        if rounded:
            W, b = fold(w, conv_name, bn_name)
            return conv(x, W, stride) + b
        y = conv(x, w[conv_name + ".weight"], stride)
        if bn_name is None:
            return y
        g, b, m, v = (w[f"{bn_name}.{k}"].astype(np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
        return (y - m) / np.sqrt(v + EPS) * g + b

    def block(x, p, stride):
        y = r(np.maximum(cb(x, p + ".conv1", p + ".bn1", stride), 0.0))
        if stride == 1:
            return r(np.maximum(cb(y, p + ".conv2", p + ".bn2") + x, 0.0))
        if not rounded:
            return np.maximum(cb(y, p + ".conv2", p + ".bn2") + cb(x, p + ".downsample.0", p + ".downsample.1", 2), 0.0)
        # one accumulator for both products, the two biases summed in float32 first
        (W2, b2), (Wd, bd) = fold(w, p + ".conv2", p + ".bn2"), fold(w, p + ".downsample.0", p + ".downsample.1")
        bias = (b2.astype(np.float32) + bd.astype(np.float32)).astype(np.float64)
        return r(np.maximum(conv(y, W2, 1) + conv(x, Wd, 2) + bias, 0.0))

    def lrelu(v):
        return np.where(v > 0, v, LRELU * v)

    x = r(np.asarray(images, np.float64))[..., None]
    x0 = r(np.maximum(cb(x, "conv1", "bn1", 2), 0.0))
    x1 = block(block(x0, "layer1.0", 1), "layer1.1", 1)
    x2 = block(block(x1, "layer2.0", 2), "layer2.1", 1)
    x3 = block(block(x2, "layer3.0", 2), "layer3.1", 1)
    x3_out = cb(x3, "layer3_outconv", None)
    t = r(cb(x2, "layer2_outconv", None) + up2(r(x3_out), rounded))
    t = r(lrelu(cb(t, "layer2_outconv2.0", "layer2_outconv2.1")))
    x2_out = r(cb(t, "layer2_outconv2.3", None))
    t = r(cb(x1, "layer1_outconv", None) + up2(x2_out, rounded))
    t = r(lrelu(cb(t, "layer1_outconv2.0", "layer1_outconv2.1")))
    x1_out = r(cb(t, "layer1_outconv2.3", None))
    return x3_out.transpose(0, 3, 1, 2), x1_out.transpose(0, 3, 1, 2)
