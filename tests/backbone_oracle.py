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


def _up2_coords(h, ft):
    y = np.arange(2 * h)
    s = (y * (h - 1)).astype(ft) / ft(2 * h - 1)
    y0 = np.floor(s).astype(np.int64)
    return y0, np.minimum(y0 + 1, h - 1), (s - y0.astype(ft)).astype(ft)


def _up2(x, coord_t, blend_t):
    _, h, w, _ = x.shape
    y0, y1, fy = _up2_coords(h, coord_t)
    x0, x1, fx = _up2_coords(w, coord_t)
    x = x.astype(blend_t)
    fy, fx = fy.astype(blend_t)[None, :, None, None], fx.astype(blend_t)[None, None, :, None]
    top = (1 - fx) * x[:, y0][:, :, x0] + fx * x[:, y0][:, :, x1]
    bot = (1 - fx) * x[:, y1][:, :, x0] + fx * x[:, y1][:, :, x1]
    return (1 - fy) * top + fy * bot


def up2(x, rounded):
    """x [N,h,w,C] -> [N,2h,2w,C], bilinear, align_corners=True, in the order the definition states."""
    ft = np.float32 if rounded else np.float64
    return _up2(x, ft, ft).astype(np.float64)


# the 20 convolutions in the order of the device's BB_LAYERS, and the names forward() traces under
LAYER_NAMES = tuple(n for n in conv_shapes() if "downsample" not in n)
TRACE_KEYS = LAYER_NAMES + ("coarse",)


def forward(w, images, rounded=False, trace=None):
    """images [N,H,W] -> (coarse [N,256,H/8,W/8], fine [N,128,H/2,W/2]) float64, the module's layout.

    trace, a dict, receives every stored activation as channels-last float64 [N,h,w,C]: the outputs of the
    20 layers under LAYER_NAMES (layer3_outconv's is the fp16 copy when rounded) and x3_out as "coarse".

    rounded=True keeps the accumulator in float64 and runs the epilogue as the device does, in float32: the
    accumulator rounded to float32, + b', + the residual, + the upsampled term, relu or 0.01f * s, then one
    rounding to fp16."""
    f32 = np.float32

    def keep(name, v):
        if trace is not None:
            trace[name] = v
        return v

    def epilogue(name, acc, b, res=None, up=None, act=None):
        """acc f64 and b' -> the stored activation of layer `name`."""
        if rounded:
            v = acc.astype(f32) + b.astype(f32)
            if res is not None:
                v = v + res.astype(f32)
            if up is not None:
                v = v + up.astype(f32)
            lr = f32(LRELU) * v
        else:
            v = acc + b + (0.0 if res is None else res) + (0.0 if up is None else up)
            lr = LRELU * v
        if act == "relu":
            v = np.maximum(v, 0)
        if act == "lrelu":
            v = np.where(v > 0, v, lr)
        return keep(name, _f16(v) if rounded else v.astype(np.float64))

    def cb(x, conv_name, bn_name, stride=1):
        """(accumulator, bias): the folded convolution when rounded, else convolution then BatchNorm."""
        if rounded:
            W, b = fold(w, conv_name, bn_name)
            return conv(x, W, stride), b
        y = conv(x, w[conv_name + ".weight"], stride)
        if bn_name is None:
            return y, 0.0
        g, b, m, v = (w[f"{bn_name}.{k}"].astype(np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
        return (y - m) / np.sqrt(v + EPS) * g + b, 0.0

    def block(x, p, stride):
        y = epilogue(p + ".conv1", *cb(x, p + ".conv1", p + ".bn1", stride), act="relu")
        a2, b2 = cb(y, p + ".conv2", p + ".bn2")
        if stride == 1:
            return epilogue(p + ".conv2", a2, b2, res=x, act="relu")
        # one accumulator for both products, the two biases summed in float32 first
        ad, bd = cb(x, p + ".downsample.0", p + ".downsample.1", 2)
        bias = (f32(b2) + f32(bd)).astype(np.float64) if rounded else 0.0
        return epilogue(p + ".conv2", a2 + ad, bias, act="relu")

    r = _f16 if rounded else (lambda v: v)
    x = r(np.asarray(images, np.float64))[..., None]
    x0 = epilogue("conv1", *cb(x, "conv1", "bn1", 2), act="relu")
    x1 = block(block(x0, "layer1.0", 1), "layer1.1", 1)
    x2 = block(block(x1, "layer2.0", 2), "layer2.1", 1)
    x3 = block(block(x2, "layer3.0", 2), "layer3.1", 1)
    x3_out = keep("coarse", cb(x3, "layer3_outconv", None)[0])
    x3_16 = keep("layer3_outconv", r(x3_out))
    t = epilogue("layer2_outconv", *cb(x2, "layer2_outconv", None), up=up2(x3_16, rounded))
    t = epilogue("layer2_outconv2.0", *cb(t, "layer2_outconv2.0", "layer2_outconv2.1"), act="lrelu")
    x2_out = epilogue("layer2_outconv2.3", *cb(t, "layer2_outconv2.3", None))
    t = epilogue("layer1_outconv", *cb(x1, "layer1_outconv", None), up=up2(x2_out, rounded))
    t = epilogue("layer1_outconv2.0", *cb(t, "layer1_outconv2.0", "layer1_outconv2.1"), act="lrelu")
    x1_out = epilogue("layer1_outconv2.3", *cb(t, "layer1_outconv2.3", None))
    return x3_out.transpose(0, 3, 1, 2), x1_out.transpose(0, 3, 1, 2)


# ---- the scratch buffer as an observation window ----

# BbScratch of csrc/backbone.hip: (name, level, the C_p the part is sized for, the C_p of the tensor it holds
# when the call returns), in the order the buffer is carved. m1 is sized for the 256 channels of
# layer2_outconv's output and ends with x2_out, 196 -> 224 channels, packed at its start.
SCRATCH_PARTS = (("s0", 2, 128, 128), ("s1", 2, 224, 224), ("s2", 2, 224, 224), ("m0", 4, 224, 224), ("m1", 4, 256, 224),
                 ("m2", 4, 256, 256), ("c0", 8, 256, 256), ("c1", 8, 256, 256), ("c2", 8, 256, 256))
# what a part holds when the call returns, as a key of forward()'s trace
SCRATCH_HOLDS = {"s0": "layer1.1.conv2", "s1": "layer1_outconv", "s2": "layer1_outconv2.0", "m0": "layer2.1.conv2",
                 "m1": "layer2_outconv2.3", "m2": "layer2_outconv2.0", "c0": "layer3.1.conv2", "c1": "layer3_outconv",
                 "c2": "layer3.0.conv2"}


def scratch_offsets(N, H, W):
    """name -> (byte offset, (N, h, w, C_p)), and the buffer's size: the parts in order, each rounded up to
    256 bytes, as bundlesdf_amd.backbone.scratch_bytes counts them."""
    out, at = {}, 0
    for name, level, sized, cp in SCRATCH_PARTS:
        pixels = N * (H // level) * (W // level)
        out[name] = (at, (N, H // level, W // level, cp))
        at += (2 * pixels * sized + 255) // 256 * 256
    return out, at


def scratch_views(scratch_uint8, N, H, W):
    """The nine activations of a call on N images of H x W as fp16 views [N,h,w,C_p] of its scratch buffer,
    a flat uint8 torch tensor or numpy array (which may be longer than the call needed)."""
    offsets, total = scratch_offsets(N, H, W)
    assert scratch_uint8.ndim == 1 and scratch_uint8.shape[0] >= total, (tuple(scratch_uint8.shape), total)
    views = {}
    for name, (at, shape) in offsets.items():
        part = scratch_uint8[at:at + 2 * int(np.prod(shape))]
        if isinstance(part, np.ndarray):
            views[name] = part.view(np.float16).reshape(shape)
        else:
            import torch
            views[name] = part.view(torch.float16).view(shape)
    return views


# ---- integer runs: every product, partial sum and stored activation exact ----

# Integer BatchNorm biases, bias[c] = base - c % 3, base per BatchNorm below: minus the 0.9 quantile of the
# pre-activation that this file's float64 forward gives on exact_images("ragged"), layer after layer, so
# that relu keeps about a tenth of the entries and the largest activation of the trunk stays below 1000.
# One channel in 32 (c % 32 == 5) has the bias 1 + c % 3 instead: it stays alive where a level is a single
# pixel and a 3x3 sum has one tap, as on the 8 x 8 case.
EXACT_BIAS = {"bn1": -8, "layer1.0.bn1": -5, "layer1.0.bn2": -6, "layer1.1.bn1": -8, "layer1.1.bn2": -9,
              "layer2.0.bn1": -13, "layer2.0.bn2": -18, "layer2.0.downsample.1": 0, "layer2.1.bn1": -21,
              "layer2.1.bn2": -33, "layer3.0.bn1": -38, "layer3.0.bn2": -71, "layer3.0.downsample.1": 0,
              "layer3.1.bn1": -85, "layer3.1.bn2": -127, "layer2_outconv2.1": -50, "layer1_outconv2.1": -13}


def exact_images(case):
    """[N,H,W] float32 integers 0..7, drawn from the case's seed."""
    c = CASES[case]
    rng = np.random.default_rng(c["seed"] + 1000)
    return rng.integers(0, 8, (c["N"], c["H"], c["W"])).astype(np.float32)


def exact_weights(kind):
    """Weights under which the device's arithmetic is exact. Every convolution is ternary: output channel o
    has one +-1 per tap t, at input channel (5 o + 37 t + 11) % Cin with sign (-1)^(o + t + o // 9), so every
    (tap, channel) column of a matrix with Cout >= Cin is hit (5 is coprime to 128, 196 and 256); the stem
    keeps the taps t with (t + 6 o) % 49 < 8 of channel o. BatchNorm is weight 1, mean 0, var float32(1 -
    1e-5): the float64 fold rounds to the same ternary W', and b' is the integer bias of EXACT_BIAS.
    kind "head" is "trunk" with layer3_outconv and layer2_outconv2.3 zero: both up2 terms are then 0 and
    layer2_outconv, layer2_outconv2.0, layer1_outconv and layer1_outconv2.0 are exact too."""
    assert kind in ("trunk", "head"), kind
    w = {}
    for name, (cout, cin, k) in conv_shapes().items():
        W = np.zeros((cout, cin, k, k), np.float32)
        o = np.arange(cout)
        for t in range(k * k):
            sign = 1.0 - 2.0 * ((o + t + o // 9) % 2)
            if cin == 1:
                sign = sign * ((t + 6 * o) % 49 < 8)
            W[o, (5 * o + 37 * t + 11) % cin, t // k, t % k] = sign
        w[name + ".weight"] = W
    for name, c in norm_shapes().items():
        w[name + ".weight"] = np.ones(c, np.float32)
        ch = np.arange(c)
        w[name + ".bias"] = np.where(ch % 32 == 5, 1 + ch % 3, EXACT_BIAS[name] - ch % 3).astype(np.float32)
        w[name + ".running_mean"] = np.zeros(c, np.float32)
        w[name + ".running_var"] = np.full(c, 1.0 - EPS, np.float32)
    if kind == "head":
        for name in ("layer3_outconv", "layer2_outconv2.3"):
            w[name + ".weight"] = np.zeros_like(w[name + ".weight"])
    return w


# ---- one layer from given inputs ----

def layer_spec(li):
    """(convolution, its BatchNorm or None, (skip convolution, its BatchNorm) or None, stride, activation) of
    layer li of LAYER_NAMES."""
    name = LAYER_NAMES[li]
    bn = None
    if li <= 12:
        bn = name.replace("conv", "bn")                             # conv1 -> bn1, layerS.B.convC -> layerS.B.bnC
    elif name.endswith("outconv2.0"):
        bn = name[:-1] + "1"
    skip = (name[:-5] + "downsample.0", name[:-5] + "downsample.1") if name in ("layer2.0.conv2", "layer3.0.conv2") else None
    stride = 2 if name in ("conv1", "layer2.0.conv1", "layer3.0.conv1") else 1
    act = "relu" if li <= 12 else "lrelu" if name.endswith("outconv2.0") else None
    return name, bn, skip, stride, act


# layer -> the layers whose outputs it reads as (input, skip, residual, up source); -1 is the image
LAYER_INPUTS = {0: (-1, None, None, None), 1: (0, None, None, None), 2: (1, None, 0, None), 3: (2, None, None, None),
                4: (3, None, 2, None), 5: (4, None, None, None), 6: (5, 4, None, None), 7: (6, None, None, None),
                8: (7, None, 6, None), 9: (8, None, None, None), 10: (9, 8, None, None), 11: (10, None, None, None),
                12: (11, None, 10, None), 13: (12, None, None, None), 14: (8, None, None, 13), 15: (14, None, None, None),
                16: (15, None, None, None), 17: (4, None, None, 16), 18: (17, None, None, None), 19: (18, None, None, None)}


def layer_inputs(li, trace, images):
    """The keyword arguments of layer_reference for layer li from a trace of forward() on images."""
    get = lambda i: None if i is None else np.asarray(images)[..., None] if i < 0 else trace[LAYER_NAMES[i]]
    x, skip, res, up = LAYER_INPUTS[li]
    return dict(x=get(x), skip=get(skip), res=get(res), up=get(up))


def layer_columns(li):
    """K of layer li: the column count of the matrix the device multiplies by, pad columns included."""
    name, _, skip, _, _ = layer_spec(li)
    pad = lambda c: (c + 31) // 32 * 32
    shapes = conv_shapes()
    _, cin, k = shapes[name]
    return 64 if cin == 1 else k * k * pad(cin) + (pad(shapes[skip[0]][1]) if skip else 0)


def layer_reference(w, li, x, skip=None, res=None, up=None):
    """Layer li alone in float64 from fp16 inputs, channels-last with or without their pad channels: x the
    input, skip the block input of a fused 1x1 stride-2 shortcut, res the residual, up the coarser map that
    up2 reads -> (the value before the final rounding to fp16 [N,ho,wo,Cout], A), A = sum |W'||x| + |b'| +
    |res| + the up2 blend of |up| per element: what the float32 rounding errors scale with. The up2
    coordinates are the definition's float32 values; everything else is float64."""
    name, bn, sk, stride, act = layer_spec(li)
    assert (sk is None) == (skip is None), name
    f64 = lambda v, c: np.asarray(v, np.float16).astype(np.float64)[..., :c]
    cout, cin, _ = conv_shapes()[name]
    W, b = fold(w, name, bn)
    x = f64(x, cin)
    v, A = conv(x, W, stride), conv(np.abs(x), np.abs(W), stride)
    if sk is not None:
        Wd, bd = fold(w, *sk)
        s = f64(skip, Wd.shape[1])
        v, A = v + conv(s, Wd, 2), A + conv(np.abs(s), np.abs(Wd), 2)
        b = (b.astype(np.float32) + bd.astype(np.float32)).astype(np.float64)
    v, A = v + b, A + np.abs(b)
    if res is not None:
        v, A = v + f64(res, cout), A + np.abs(f64(res, cout))
    if up is not None:
        u = f64(up, cout)
        v, A = v + _up2(u, np.float32, np.float64), A + _up2(np.abs(u), np.float32, np.float64)
    if act == "relu":
        v = np.maximum(v, 0.0)
    if act == "lrelu":
        v = np.where(v > 0, v, float(np.float32(LRELU)) * v)
    return v, A


def layer_bound(li, got, ref, A, half=True):
    """The isolation bound per element: half an fp16 ulp of the larger of got and ref (normal and
    subnormal) when the value was stored as fp16, plus (K + 8) 2^-23 A for a float32 sum of K exact products
    in any order and either MFMA rounding mode and the epilogue's few operations."""
    ulp = 2.0 ** -11 * np.maximum(np.abs(got), np.abs(ref)) + 2.0 ** -24 if half else 0.0
    return ulp + (layer_columns(li) + 8) * 2.0 ** -23 * A


