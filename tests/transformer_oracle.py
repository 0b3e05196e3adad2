"""Float64 numpy restatement of the feature transformer's definition (the header comment of
bundlesdf_amd/csrc/feature_transformer.hip), with the generators of the weights, inputs and masks
the tests and tests/golden/make_feature_transformer.py share. Nothing here is stored: weights and
inputs are drawn again from their seeds wherever they are needed.

One application x <- layer(x, source), H = 8 heads of D = C/8:
    Q = elu(x Wq^T) + 1, K = elu(source Wk^T) + 1, V = source Wv^T, masked rows zeroed
    KV_h = (1/S) sum_s K_h[s]^T V_h[s], Ksum_h = sum_s K_h[s]
    msg_h[l] = (Q_h[l] KV_h) S / (Q_h[l] . Ksum_h + 1e-6)
    m = LN1(msg Wm^T); m = LN2(relu([x | m] W1^T) W2^T); out = x + m

layer and forward take mutant=: one named one-line deviation from that definition (MUTANTS below). The
tests use them to show that a case can tell the deviation from the definition (CPU), and that the
kernels' error has no component along it (GPU).
"""
import functools

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
    # Edge shapes: 64 | L, one row past a tile, one row past one and two 256-row KV blocks, the D = 16 path over
    # several blocks, a self layer whose sides have 2 and 1 KV blocks. stored=False: the fixture holds only their
    # e16; the float64 outputs are the oracle's, computed where they are needed.
    "edge_64_65": dict(C=256, layers=("cross",), P=2, L=64, S=65, masks="random", seed=111, stored=False),
    "edge_257_513": dict(C=256, layers=("cross",), P=2, L=257, S=513, masks="random", seed=112, stored=False),
    "fine_128_257": dict(C=128, layers=("cross",), P=2, L=128, S=257, masks="random", seed=113, stored=False),
    "fine_self_300_45": dict(C=128, layers=("self",), P=2, L=300, S=45, masks="random", seed=114, stored=False),
    "fine_65_513": dict(C=128, layers=("self", "cross"), P=2, L=65, S=513, masks="random", seed=115, stored=False),
    # Amplifying cases: merge.weight and mlp.2.weight scaled by a power of two so that the variance LayerNorm1 and
    # LayerNorm2 see is of the order of their eps, 1e-5. Only there does eps show in the output.
    "amp256": dict(C=256, layers=("cross",), P=2, L=70, S=45, masks="none", seed=116, stored=False,
                   scale={"merge.weight": 2.0 ** -6, "mlp.2.weight": 2.0 ** -8}),
    "amp128": dict(C=128, layers=("self",), P=2, L=70, S=45, masks="none", seed=117, stored=False,
                   scale={"merge.weight": 2.0 ** -6, "mlp.2.weight": 2.0 ** -8}),
}
STORED = [k for k, c in CASES.items() if c.get("stored", True)]
KV_ROWS = 256                                   # FT_KV_ROWS of csrc/feature_transformer.hip: rows of a KV partial

# mutant -> (the cases that must tell it from the definition, the distance they must reach in e16_rms).
# 6 x: the structural ones, which by the triangle inequality cannot pass the kernels' 2 x e16 bound; 1 x: a wrong
# constant or divisor, which that bound alone does not see and the projection test is there for.
MUTANTS = {
    "ln1_eps": (("amp256", "amp128"), 1),
    "ln2_eps": (("amp256", "amp128"), 1),
    "ln1_unbiased": (("self1", "fine_128_257"), 1),
    "ln2_unbiased": (("self1", "fine_128_257"), 1),
    "ln_swap": (("self1", "fine_128_257"), 1),
    "k_no_plus1": (("cross1", "fine_128_257"), 1),
    "no_q_mask": (("edge_64_65", "fine_self_300_45"), 6),
    "no_k_mask": (("edge_64_65", "fine_self_300_45"), 6),
    "mx_swap": (("self1", "fine_128_257"), 6),
    "heads_leak": (("fine_128_257", "fine_self_300_45"), 6),
    "drop_row:63": (("edge_257_513", "fine_128_257"), 6),
    "drop_row:64": (("edge_257_513", "fine_128_257"), 6),
    "drop_row:255": (("edge_257_513", "fine_128_257"), 6),
    "drop_row:256": (("edge_257_513", "fine_128_257"), 6),
    "drop_row:last": (("edge_257_513", "fine_128_257", "edge_64_65"), 6),
    "drop_block:1": (("edge_257_513", "fine_128_257"), 6),
    "drop_block:2": (("edge_257_513",), 6),
    "cross_b_first": (("cross1", "edge_64_65"), 6),
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


def make_weights(seed, d_model, layer_names, scale=None):
    """The reference's parameter names -> float32 arrays of fp16 values. Matrices uniform in
    +-sqrt(6 / (fan_in + fan_out)); LayerNorm weight 1 + 0.1 N(0,1), bias 0.1 N(0,1). scale maps the
    end of a key to a factor applied before the rounding to fp16."""
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
            for end, f in (scale or {}).items():
                if key.endswith(end):
                    v = v * f
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
    w = make_weights(c["seed"], c["C"], c["layers"], c.get("scale"))
    a, b = make_inputs(c["seed"] + 1000, c["P"], c["L"], c["S"], c["C"])
    return (w, a, b) + make_masks(case)


def _layernorm(x, g, b, eps=EPS_LN, unbiased=False):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).sum(-1, keepdims=True) / (x.shape[-1] - (1 if unbiased else 0))
    return (x - mu) / np.sqrt(var + eps) * g + b


def layer(w, i, x, src, x_mask=None, src_mask=None, mutant=None):
    """One application on one problem: x [L,C], src [S,C] float64. mutant: a key of MUTANTS (a row or block
    that the source does not have is not dropped)."""
    g = lambda name: w[f"layers.{i}.{name}"].astype(np.float64)
    kind, _, arg = (mutant or "").partition(":")
    L, C = x.shape
    S, D = src.shape[0], C // H
    elu1 = lambda v: np.where(v > 0, v + 1.0, np.exp(np.minimum(v, 0.0)))
    Q, K, V = elu1(x @ g("q_proj.weight").T), elu1(src @ g("k_proj.weight").T), src @ g("v_proj.weight").T
    if kind == "k_no_plus1":
        K = K - 1.0
    if x_mask is not None and kind != "no_q_mask":
        Q = Q * x_mask[:, None]
    if src_mask is not None:
        K, V = (K if kind == "no_k_mask" else K * src_mask[:, None]), V * src_mask[:, None]
    if kind == "drop_row":
        r = S - 1 if arg == "last" else int(arg)
        if r < S:
            K, V = K.copy(), V.copy()
            K[r], V[r] = 0.0, 0.0
    if kind == "drop_block":
        K, V = K.copy(), V.copy()
        K[KV_ROWS * int(arg):KV_ROWS * (int(arg) + 1)], V[KV_ROWS * int(arg):KV_ROWS * (int(arg) + 1)] = 0.0, 0.0
    Q, K, V = Q.reshape(L, H, D), K.reshape(S, H, D), V.reshape(S, H, D)
    Z = np.einsum("lhd,hd->lh", Q, K.sum(0))
    if kind == "heads_leak" and D == 16:            # the 32 x 32 product of two heads, its off-diagonal blocks kept
        KV = np.einsum("sgd,sge->gde", K.reshape(S, H // 2, 32), V.reshape(S, H // 2, 32)) / S
        msg = np.einsum("lgd,gde->lge", Q.reshape(L, H // 2, 32), KV).reshape(L, H, D)
    else:
        KV = np.einsum("shd,she->hde", K, V) / S
        msg = np.einsum("lhd,hde->lhe", Q, KV)
    msg = msg * (S / (Z + EPS_Z))[:, :, None]
    n1, n2 = ("norm2", "norm1") if kind == "ln_swap" else ("norm1", "norm2")
    m = _layernorm(msg.reshape(L, C) @ g("merge.weight").T, g(n1 + ".weight"), g(n1 + ".bias"),
                   1e-6 if kind == "ln1_eps" else EPS_LN, kind == "ln1_unbiased")
    hid = np.maximum(np.concatenate([m, x] if kind == "mx_swap" else [x, m], 1) @ g("mlp.0.weight").T, 0.0)
    return x + _layernorm(hid @ g("mlp.2.weight").T, g(n2 + ".weight"), g(n2 + ".bias"),
                          1e-6 if kind == "ln2_eps" else EPS_LN, kind == "ln2_unbiased")


def forward(w, layer_names, feat_a, feat_b, mask_a=None, mask_b=None, cross_b_first=False, mutant=None):
    """The stack on P pairs -> (out_a, out_b) float64. cross_b_first (or mutant="cross_b_first") applies the
    two halves of every cross layer in the other order (b first, then a from the updated b): the bug the
    cross1 case is there to catch. Any other mutant goes to every layer application."""
    cross_b_first = cross_b_first or mutant == "cross_b_first"
    mut = None if mutant == "cross_b_first" else mutant
    P = feat_a.shape[0]
    out_a, out_b = [], []
    for p in range(P):
        a, b = feat_a[p].astype(np.float64), feat_b[p].astype(np.float64)
        ma = None if mask_a is None else mask_a[p].astype(np.float64)
        mb = None if mask_b is None else mask_b[p].astype(np.float64)
        for i, name in enumerate(layer_names):
            if name == "self":
                a, b = layer(w, i, a, a, ma, ma, mut), layer(w, i, b, b, mb, mb, mut)
            elif name == "cross" and not cross_b_first:
                a = layer(w, i, a, b, ma, mb, mut)
                b = layer(w, i, b, a, mb, ma, mut)
            elif name == "cross":
                b = layer(w, i, b, a, mb, ma, mut)
                a = layer(w, i, a, b, ma, mb, mut)
            else:
                raise KeyError(name)
        out_a.append(a)
        out_b.append(b)
    return np.stack(out_a), np.stack(out_b)


@functools.lru_cache(maxsize=None)
def case_output(case, masked=False, mutant=None):
    """(out_a, out_b) of the oracle (or of a mutant) on a case, with or without the case's masks. Cached and
    shared: do not write into it."""
    w, a, b, ma, mb = case_data(case)
    out = forward(w, CASES[case]["layers"], a, b, ma if masked else None, mb if masked else None, mutant=mutant)
    for o in out:
        o.setflags(write=False)
    return out


def flat(out):
    """Both outputs as one float64 vector."""
    return np.concatenate([np.asarray(out[0], np.float64).ravel(), np.asarray(out[1], np.float64).ravel()])


def mutant_delta(case, mutant):
    """d_m = mutant output - oracle output over both outputs, with the case's masks where it has them."""
    masked = CASES[case]["masks"] != "none"
    return flat(case_output(case, masked, mutant)) - flat(case_output(case, masked))


def projection(err, d):
    """alpha = <err, d> / <d, d>: 1 if err is the deviation d itself, about (rms(err) / rms(d)) / sqrt(n) for
    zero-mean noise."""
    return float(err @ d / (d @ d))
