"""Float64 numpy restatement of the feature transformer's definition (the header comment of
bundlesdf_amd/csrc/feature_transformer.hip), with the generators of the weights, inputs and masks
the tests and tests/golden/make_feature_transformer.py share. Nothing here is stored: weights and
inputs are drawn again from their seeds wherever they are needed.

One application x <- layer(x, source), H = 8 heads of D = C/8:
    Q = elu(x Wq^T) + 1, K = elu(source Wk^T) + 1, V = source Wv^T, masked rows zeroed
    KV_h = (1/S) sum_s K_h[s]^T V_h[s], Ksum_h = sum_s K_h[s]
    msg_h[l] = (Q_h[l] KV_h) S / (Q_h[l] . Ksum_h + 1e-6)
    m = LN1(msg Wm^T); m = LN2(relu([x | m] W1^T) W2^T); out = x + m
"""
import numpy as np

H = 8
EPS_Z = 1e-6
EPS_LN = 1e-5

# name -> C, layer names, P, L, S, hw_a, hw_b, masks ("none", "random", "dead"), seed
CASES = {
    "coarse8": dict(C=256, layers=("self", "cross") * 4, P=2, L=70, S=45, masks="random", seed=101),
    "self1": dict(C=256, layers=("self",), P=2, L=70, S=45, masks="none", seed=102),
    "cross1": dict(C=256, layers=("cross",), P=2, L=40, S=300, masks="none", seed=103),
    "fine2": dict(C=128, layers=("self", "cross"), P=5, L=25, S=25, masks="none", seed=104),
    "one": dict(C=256, layers=("self", "cross"), P=1, L=1, S=1, masks="none", seed=105),
    "dead": dict(C=256, layers=("self", "cross"), P=2, L=40, S=45, masks="dead", seed=106),
}
PE_GRIDS = ((256, 7, 10), (128, 5, 9))          # (C, h, w) of the position-encoding crops


SHARD_BYTES = 900_000                           # array bytes per fixture shard (float64 does not compress)


def shard_name(i):
    return "feature_transformer.npz" if i == 0 else f"feature_transformer.{i}.npz"


def load_golden(golden_dir):
    """tests/golden/feature_transformer*.npz as one dict; the per-pair parts "key@p" stacked to [P,n,C]."""
    import os
    first = np.load(os.path.join(golden_dir, shard_name(0)))
    flat = {}
    for i in range(int(first["n_shards"])):
        with np.load(os.path.join(golden_dir, shard_name(i))) as z:
            flat.update({k: z[k] for k in z.files})
    out, pairs = {}, {}
    for k, v in flat.items():
        if "@" in k:
            key, p = k.split("@")
            pairs.setdefault(key, {})[int(p)] = v
        else:
            out[k] = v
    for key, d in pairs.items():
        out[key] = np.stack([d[p] for p in range(len(d))])
    return out


def _f16(x):
    return x.astype(np.float16).astype(np.float32)


def layer_keys(i, C):
    p = f"layers.{i}."
    return [(p + "q_proj.weight", (C, C)), (p + "k_proj.weight", (C, C)), (p + "v_proj.weight", (C, C)),
            (p + "merge.weight", (C, C)), (p + "mlp.0.weight", (2 * C, 2 * C)), (p + "mlp.2.weight", (C, 2 * C)),
            (p + "norm1.weight", (C,)), (p + "norm1.bias", (C,)), (p + "norm2.weight", (C,)), (p + "norm2.bias", (C,))]


def make_weights(seed, d_model, layer_names):
    """The reference's parameter names -> float32 arrays of fp16 values. Matrices uniform in
    +-sqrt(6 / (fan_in + fan_out)); LayerNorm weight 1 + 0.1 N(0,1), bias 0.1 N(0,1)."""
    rng = np.random.default_rng(seed)
    w = {}
    for i in range(len(layer_names)):
        for key, shape in layer_keys(i, d_model):
            if len(shape) == 2:
                bound = np.sqrt(6.0 / (shape[0] + shape[1]))
                v = rng.uniform(-bound, bound, size=shape)
            elif key.endswith("weight"):
                v = 1.0 + 0.1 * rng.standard_normal(shape)
            else:
                v = 0.1 * rng.standard_normal(shape)
            w[key] = _f16(v)
    return w


def make_inputs(seed, P, L, S, C):
    """(feat_a [P,L,C], feat_b [P,S,C]) standard normal, float32 arrays of fp16 values."""
    rng = np.random.default_rng(seed)
    return _f16(rng.standard_normal((P, L, C))), _f16(rng.standard_normal((P, S, C)))


def make_masks(case):
    """(mask_a [P,L], mask_b [P,S]) bool, or (None, None). "random" keeps 80 %; "dead" has a random
    mask_a and pair 1's mask_b all false."""
    c = CASES[case]
    if c["masks"] == "none":
        return None, None
    rng = np.random.default_rng(c["seed"] + 5000)
    ma = rng.random((c["P"], c["L"])) < 0.8
    mb = rng.random((c["P"], c["S"])) < 0.8
    if c["masks"] == "dead":
        mb[1, :] = False
    return ma, mb


def case_data(case):
    """(weights, feat_a, feat_b, mask_a, mask_b) of a case."""
    c = CASES[case]
    w = make_weights(c["seed"], c["C"], c["layers"])
    a, b = make_inputs(c["seed"] + 1000, c["P"], c["L"], c["S"], c["C"])
    return (w, a, b) + make_masks(case)


def _layernorm(x, g, b):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + EPS_LN) * g + b


def layer(w, i, x, src, x_mask=None, src_mask=None):
    """One application on one problem: x [L,C], src [S,C] float64."""
    g = lambda name: w[f"layers.{i}.{name}"].astype(np.float64)
    L, C = x.shape
    S, D = src.shape[0], C // H
    elu1 = lambda v: np.where(v > 0, v + 1.0, np.exp(np.minimum(v, 0.0)))
    Q, K, V = elu1(x @ g("q_proj.weight").T), elu1(src @ g("k_proj.weight").T), src @ g("v_proj.weight").T
    if x_mask is not None:
        Q = Q * x_mask[:, None]
    if src_mask is not None:
        K, V = K * src_mask[:, None], V * src_mask[:, None]
    Q, K, V = Q.reshape(L, H, D), K.reshape(S, H, D), V.reshape(S, H, D)
    KV = np.einsum("shd,she->hde", K, V) / S
    Z = np.einsum("lhd,hd->lh", Q, K.sum(0))
    msg = np.einsum("lhd,hde->lhe", Q, KV) * (S / (Z + EPS_Z))[:, :, None]
    m = _layernorm(msg.reshape(L, C) @ g("merge.weight").T, g("norm1.weight"), g("norm1.bias"))
    hid = np.maximum(np.concatenate([x, m], 1) @ g("mlp.0.weight").T, 0.0)
    return x + _layernorm(hid @ g("mlp.2.weight").T, g("norm2.weight"), g("norm2.bias"))


def forward(w, layer_names, feat_a, feat_b, mask_a=None, mask_b=None, cross_b_first=False):
    """The stack on P pairs -> (out_a, out_b) float64. cross_b_first applies the two halves of every
    cross layer in the other order (b first, then a from the updated b): the bug the cross1 case is
    there to catch."""
    P = feat_a.shape[0]
    out_a, out_b = [], []
    for p in range(P):
        a, b = feat_a[p].astype(np.float64), feat_b[p].astype(np.float64)
        ma = None if mask_a is None else mask_a[p].astype(np.float64)
        mb = None if mask_b is None else mask_b[p].astype(np.float64)
        for i, name in enumerate(layer_names):
            if name == "self":
                a, b = layer(w, i, a, a, ma, ma), layer(w, i, b, b, mb, mb)
            elif name == "cross" and not cross_b_first:
                a = layer(w, i, a, b, ma, mb)
                b = layer(w, i, b, a, mb, ma)
            elif name == "cross":
                b = layer(w, i, b, a, mb, ma)
                a = layer(w, i, a, b, ma, mb)
            else:
                raise KeyError(name)
        out_a.append(a)
        out_b.append(b)
    return np.stack(out_a), np.stack(out_b)
