"""Feature transformer on the device: fused linear-attention layers.

What stands between a backbone and match_descriptors. In the reference LoFTR.forward adds a
sinusoidal position encoding to the coarse feature maps, flattens them to [N, hw, C] and runs
LocalFeatureTransformer (BundleTrack/LoFTR/src/loftr/loftr_module/transformer.py: LoFTREncoderLayers
alternating "self" and "cross", each a multi-head linear attention and a feed-forward block) before
the matching head sees them. Here the stack is nof_feature_transformer (csrc/feature_transformer.hip,
include/nof.h group 12): per layer application one kernel forms KV and Ksum of the source and one
takes a tile of 64 tokens through the rest of the layer on chip. The header comment of
csrc/feature_transformer.hip is the definition; tests/transformer_oracle.py restates it in float64.

No CPU fallback: FeatureTransformer.forward raises if libnof.so cannot run. The position encoding
is plumbing written with torch ops and runs anywhere. The chain is
add_position_encoding -> FeatureTransformer.forward -> match_descriptors -> to_pixels -> lift_matches.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._args import PackedWeights, as_host, as_tensor, default_device

__all__ = ["FeatureTransformer", "position_encoding", "add_position_encoding", "pack_matrix", "layer_bytes",
           "D_MODELS", "MAX_LAYERS", "MAX_PAIRS", "N_HEADS", "TILE"]

D_MODELS = (128, 256)
MAX_LAYERS = _lib.FT_MAX_LAYERS
MAX_PAIRS = 32767           # 2 P problems on a grid axis of 65535
N_HEADS = 8
TILE = (64, 256)            # FT_ROWS, FT_KV_ROWS of csrc/feature_transformer.hip

_KINDS = {"self": _lib.FT_SELF, "cross": _lib.FT_CROSS}
_PROBE = "layers.0.q_proj.weight"


def position_encoding(h, w, C, temp_bug_fix=False, device=None):
    """The reference's PositionEncodingSine cropped to an h x w grid, as [h w, C] float32, row-major.

    Channel 4 k + {0,1,2,3} of cell (y, x) is sin((x+1) f_k), cos((x+1) f_k), sin((y+1) f_k),
    cos((y+1) f_k) with f_k = exp(2 k d). temp_bug_fix=True has d = -ln(10000) / (C / 2); False, the
    form BundleSDF's default config and the released outdoor weights use, has d = -1: there the
    reference writes -ln(10000) / C // 2, which is a floor division of a small negative number."""
    h, w, C = int(h), int(w), int(C)
    if h < 1 or w < 1:
        raise ValueError(f"position_encoding: the grid {h}x{w} must be at least 1x1")
    if C < 4 or C % 4:
        raise ValueError(f"position_encoding: C={C} must be a positive multiple of 4")
    d = -math.log(10000.0) / (C // 2) if temp_bug_fix else -math.log(10000.0) / C // 2
    f = torch.exp(torch.arange(0, C // 2, 2).float() * d)                # [C/4]
    xs = torch.arange(1, w + 1).float()[None, :, None] * f               # [1,w,C/4]
    ys = torch.arange(1, h + 1).float()[:, None, None] * f               # [h,1,C/4]
    pe = torch.stack([torch.sin(xs).expand(h, w, -1), torch.cos(xs).expand(h, w, -1),
                      torch.sin(ys).expand(h, w, -1), torch.cos(ys).expand(h, w, -1)], dim=3)   # [h,w,C/4,4]
    pe = pe.reshape(h * w, C)
    return pe if device is None else pe.to(device)


def add_position_encoding(feat, temp_bug_fix=False):
    """feat [P,C,h,w] (array or tensor, a backbone's coarse map) -> [P, h w, C] float32 on feat's device:
    the encoding added, then the reference's rearrange 'n c h w -> n (h w) c'."""
    t = as_tensor(feat)
    if t.dim() != 4 or not t.is_floating_point():
        raise ValueError(f"add_position_encoding: feat must be a floating-point [P,C,h,w], got {tuple(t.shape)} {t.dtype}")
    P, C, h, w = t.shape
    pe = position_encoding(h, w, C, temp_bug_fix, device=t.device)
    return t.float().permute(0, 2, 3, 1).reshape(P, h * w, C) + pe[None]


def pack_matrix(W):
    """W [N,K] float16 (out, in) -> the fragment order csrc/mfma_tile.h defines, [N/32][K/16][64][8]."""
    N, K = W.shape
    return np.ascontiguousarray(W.reshape(N // 32, 32, K // 16, 2, 8).transpose(0, 2, 3, 1, 4))


def layer_bytes(C):
    return 20 * C * C + 16 * C


def _layer_keys(i, C):
    """(key, shape) of layer i in the order of the packed block."""
    p = f"layers.{i}."
    return [(p + "q_proj.weight", (C, C)), (p + "k_proj.weight", (C, C)), (p + "v_proj.weight", (C, C)),
            (p + "merge.weight", (C, C)), (p + "mlp.0.weight", (2 * C, 2 * C)), (p + "mlp.2.weight", (C, 2 * C)),
            (p + "norm1.weight", (C,)), (p + "norm1.bias", (C,)), (p + "norm2.weight", (C,)), (p + "norm2.bias", (C,))]


class FeatureTransformer(PackedWeights):
    """The stack of linear-attention layers with its weights packed for the device.

    weights maps the reference's parameter names (layers.{i}.{q_proj,k_proj,v_proj,merge}.weight,
    layers.{i}.mlp.{0,2}.weight, layers.{i}.norm{1,2}.{weight,bias}) to arrays or tensors. The matrices
    are rounded once to float16 and put in fragment order, the LayerNorm parameters stay float32,
    and everything is one buffer (.packed, uint8) that goes to the device once: at construction when
    device is given, else at the first forward."""

    def __init__(self, weights, d_model=256, layer_names=("self", "cross") * 4, device=None, prefix=""):
        what = "FeatureTransformer"
        C = int(d_model)
        if C not in D_MODELS:
            raise ValueError(f"{what}: d_model={d_model} must be one of {D_MODELS} ({N_HEADS} heads of 16 or 32)")
        names = tuple(layer_names)
        if not 1 <= len(names) <= MAX_LAYERS:
            raise ValueError(f"{what}: {len(names)} layers (1 .. {MAX_LAYERS})")
        for n in names:
            if n not in _KINDS:
                raise ValueError(f"{what}: layer name {n!r} must be 'self' or 'cross'")
        parts = []
        for i in range(len(names)):
            for key, shape in _layer_keys(i, C):
                v = self.lookup(weights, prefix, key, shape, what)
                if len(shape) == 2:
                    parts.append(pack_matrix(v.astype(np.float16)).view(np.uint8).ravel())
                else:
                    parts.append(np.ascontiguousarray(v.astype(np.float32)).view(np.uint8).ravel())
        self.d_model, self.layer_names = C, names
        super().__init__(np.concatenate(parts), device)
        assert self.packed.size == len(names) * layer_bytes(C)
        self._workspace = self._buffers         # the name tests and scripts read

    @classmethod
    def from_state_dict(cls, sd, prefix=None, d_model=256, layer_names=("self", "cross") * 4, device=None):
        """From a checkpoint's state dict. prefix is what stands before 'layers.0...' ('', 'loftr_coarse.',
        'loftr_fine.', 'matcher.loftr_coarse.', ...); None finds it: the one prefix whose first query
        projection is [d_model, d_model]."""
        if prefix is None:
            fit = [k[:-len(_PROBE)] for k in sd if k.endswith(_PROBE)
                   and tuple(as_host(sd[k]).shape) == (int(d_model), int(d_model))]
            # a lone prefix of another shape is taken too: the shape check in __init__ names the key
            prefix = fit[0] if len(fit) == 1 else cls.find_prefix(sd, _PROBE, "FeatureTransformer", "a transformer")
        return cls(sd, d_model=d_model, layer_names=layer_names, device=device, prefix=prefix)

    def _stream(self, f, name):
        t = as_tensor(f)
        if not t.is_floating_point():
            raise ValueError(f"FeatureTransformer.forward: {name} must be a floating-point array, got {t.dtype}")
        if t.dim() not in (2, 3):
            raise ValueError(f"FeatureTransformer.forward: {name} must be [n,C] or [P,n,C], got {tuple(t.shape)}")
        single = t.dim() == 2
        return (t[None] if single else t), single

    def forward(self, feat_a, feat_b, mask_a=None, mask_b=None):
        """feat_a [P,L,C], feat_b [P,S,C] (arrays or tensors, float16 or float32; one [L,C] / [S,C] pair
        comes back as P = 1), mask_a [P,L] / mask_b [P,S] (any dtype, 0 = the token takes no part, each
        optional) -> (out_a [P,L,C], out_b [P,S,C]) float32 device tensors, what match_descriptors takes."""
        what = "FeatureTransformer.forward"
        a, single = self._stream(feat_a, "feat_a")
        b, single_b = self._stream(feat_b, "feat_b")
        if single != single_b:
            raise ValueError(f"{what}: give feat_a and feat_b both with the P axis or both without")
        P, L, C = a.shape
        if b.shape[0] != P or b.shape[2] != C:
            raise ValueError(f"{what}: feat_a is {tuple(a.shape)} and feat_b {tuple(b.shape)}: P and C must agree")
        S = b.shape[1]
        if C != self.d_model:
            raise ValueError(f"{what}: C={C} but the weights are for d_model={self.d_model}")
        if P < 1 or P > MAX_PAIRS:
            raise ValueError(f"{what}: {P} pairs (1 .. {MAX_PAIRS})")
        if L < 1 or S < 1:
            raise ValueError(f"{what}: L={L} and S={S} must be at least 1")
        dev = default_device(a if a.is_cuda else b)
        masks = []
        for m, n, name in ((mask_a, L, "mask_a"), (mask_b, S, "mask_b")):
            if m is None:
                masks.append(None)
                continue
            t = as_tensor(m)
            t = t[None] if (single and t.dim() == 1) else t
            if tuple(t.shape) != (P, n):
                raise ValueError(f"{what}: {name} must be {[P, n]}, got {tuple(t.shape)}")
            masks.append((t != 0).to(torch.uint8).contiguous())

        with torch.cuda.device(dev):
            # the kernels update the streams in place: these float32 copies are the outputs
            out_a = a.to(device=dev, dtype=torch.float32, copy=True).contiguous()
            out_b = b.to(device=dev, dtype=torch.float32, copy=True).contiguous()
            ma, mb = (None if m is None else m.to(dev) for m in masks)
            self._launch(out_a, out_b, ma, mb, what)
        return out_a, out_b

    def _launch(self, a, b, mask_a, mask_b, what):
        """nof_feature_transformer on a [P,L,C] and b [P,S,C], contiguous float32 on one device (the current
        one), in place; mask_a / mask_b [P,L] / [P,S] u8 there, or None."""
        P, L, C = a.shape
        S = b.shape[1]
        lib = _lib.lib()
        w = self.device_weights(a.device)
        ws = self.buffer(w.device, int(lib.nof_feature_transformer_workspace_bytes(P, L, S, C)))
        D = _lib.FeatureTransformerDesc()
        D.feat_a, D.feat_b, D.mask_a, D.mask_b = (_lib.ptr(x) for x in (a, b, mask_a, mask_b))
        D.P, D.L, D.S, D.C, D.n_layers = P, L, S, C, len(self.layer_names)
        for i, n in enumerate(self.layer_names):
            D.layer_kind[i] = _KINDS[n]
        D.weights, D.weights_bytes = _lib.ptr(w), w.numel()
        D.workspace, D.workspace_bytes = _lib.ptr(ws), ws.numel()
        _lib.check(lib.nof_feature_transformer(ctypes.byref(D), _lib.stream_of(a)), what)

    def forward_inplace(self, a, b):
        """The stack on a [P,L,C] and b [P,S,C], contiguous float32 tensors on one device, updated where
        they lie: forward without its copies of the inputs and without masks. Returns (a, b)."""
        what = "FeatureTransformer.forward_inplace"
        for t, name in ((a, "a"), (b, "b")):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 3 or not t.is_contiguous():
                raise ValueError(f"{what}: {name} must be a contiguous float32 [P,n,C] tensor")
        P, L, C = a.shape
        S = b.shape[1]
        if b.shape[0] != P or b.shape[2] != C:
            raise ValueError(f"{what}: a is {tuple(a.shape)} and b {tuple(b.shape)}: P and C must agree")
        if C != self.d_model:
            raise ValueError(f"{what}: C={C} but the weights are for d_model={self.d_model}")
        if P < 1 or P > MAX_PAIRS:
            raise ValueError(f"{what}: {P} pairs (1 .. {MAX_PAIRS})")
        if L < 1 or S < 1:
            raise ValueError(f"{what}: L={L} and S={S} must be at least 1")
        if not a.is_cuda or a.device != b.device:
            raise ValueError(f"{what}: a is on {a.device} and b on {b.device}: one device is needed")
        with torch.cuda.device(a.device):
            self._launch(a, b, None, None, what)
        return a, b

    __call__ = forward
