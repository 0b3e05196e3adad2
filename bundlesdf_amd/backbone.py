"""LoFTR backbone on the device: fused ResNet-FPN convolutions on MFMA.

The first stage of the reference's matcher: ResNetFPN_8_2 (BundleTrack/LoFTR/src/loftr/backbone/
resnet_fpn.py) in eval mode with initial_dim = 128 and block_dims = [128, 196, 256], from grey images to
the 1/8-resolution coarse map and the 1/2-resolution fine map. Here it is nof_backbone
(csrc/backbone.hip, include/nof.h group 14): twenty launches of implicit-GEMM convolutions with
BatchNorm folded into their weights. The header comment of csrc/backbone.hip is the definition;
tests/backbone_oracle.py restates it in float64.

No CPU fallback: Backbone.forward raises if libnof.so cannot run. fold_batchnorm and pack_conv are the
statement of the weight layout on this side and run anywhere. The chain is
Backbone.forward -> FeatureTransformer.forward -> match_descriptors -> FineRefiner.refine (loftr.Loftr).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import transformer as _T
from ._args import PackedWeights, as_tensor, default_device
from .transformer import pack_matrix

__all__ = ["Backbone", "fold_batchnorm", "conv_matrix", "pack_conv", "pad_channels", "weight_layout", "scratch_bytes",
           "LAYERS", "BN_EPS", "C_COARSE", "C_FINE", "MAX_SIDE", "STEM_K"]

BN_EPS = 1e-5
C_COARSE = 256
C_FINE = 128
MAX_SIDE = 4096
STEM_K = 64             # the stem's 49 taps, padded

# (convolution, its BatchNorm or None, (skip convolution, its BatchNorm) or None) in the order of the weight
# buffer: BB_LAYERS of csrc/backbone.hip
LAYERS = (("conv1", "bn1", None),) + tuple(
    (f"layer{s}.{b}.conv{c}", f"layer{s}.{b}.bn{c}",
     (f"layer{s}.0.downsample.0", f"layer{s}.0.downsample.1") if (s > 1 and b == 0 and c == 2) else None)
    for s in (1, 2, 3) for b in (0, 1) for c in (1, 2)) + (
    ("layer3_outconv", None, None),
    ("layer2_outconv", None, None), ("layer2_outconv2.0", "layer2_outconv2.1", None), ("layer2_outconv2.3", None, None),
    ("layer1_outconv", None, None), ("layer1_outconv2.0", "layer1_outconv2.1", None), ("layer1_outconv2.3", None, None))
# convolution -> (Cout, Cin, KH)
_SHAPES = {"conv1": (128, 1, 7), "layer3_outconv": (256, 256, 1),
           "layer2_outconv": (256, 196, 1), "layer2_outconv2.0": (256, 256, 3), "layer2_outconv2.3": (196, 256, 3),
           "layer1_outconv": (196, 128, 1), "layer1_outconv2.0": (196, 196, 3), "layer1_outconv2.3": (128, 196, 3)}
for _s, (_cin, _c) in {1: (128, 128), 2: (128, 196), 3: (196, 256)}.items():
    _SHAPES.update({f"layer{_s}.0.conv1": (_c, _cin, 3), f"layer{_s}.0.conv2": (_c, _c, 3), f"layer{_s}.1.conv1": (_c, _c, 3),
                    f"layer{_s}.1.conv2": (_c, _c, 3), f"layer{_s}.0.downsample.0": (_c, _cin, 1)})
_PROBE = "layer3_outconv.weight"


def pad_channels(c):
    """The channel count as the device stores it: the next multiple of 32."""
    return (int(c) + 31) // 32 * 32


def fold_batchnorm(W, gamma, beta, mean, var, eps=BN_EPS):
    """An eval-mode BatchNorm after the bias-free convolution W [Cout,Cin,KH,KW], folded in float64 ->
    (W' float16, b' float32): W' = W gamma / sqrt(var + eps) per output channel, rounded once;
    b' = beta - mean gamma / sqrt(var + eps)."""
    s = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    Wf = np.asarray(W, np.float64) * s[:, None, None, None]
    return Wf.astype(np.float16), (np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * s).astype(np.float32)


def conv_matrix(W, skip=None):
    """W [Cout,Cin,KH,KW] float16 -> the matrix [Cout_p, K] float16 the device multiplies by: K = KH KW Cin_p,
    k = (ky KW + kx) Cin_p + c, pad rows and columns 0. The one-channel 7x7 stem has its 49 taps padded to
    STEM_K. skip [Cout,Cs,1,1], a block's 1x1 stride-2 shortcut, follows as Cs_p further columns."""
    Cout, Cin, KH, KW = W.shape
    Cout_p = pad_channels(Cout)
    if Cin == 1:
        M = np.zeros((Cout_p, STEM_K), np.float16)
        M[:Cout, :KH * KW] = W.reshape(Cout, KH * KW)
        return M
    Cin_p = pad_channels(Cin)
    M = np.zeros((Cout_p, KH * KW, Cin_p), np.float16)
    M[:Cout, :, :Cin] = W.transpose(0, 2, 3, 1).reshape(Cout, KH * KW, Cin)
    M = M.reshape(Cout_p, KH * KW * Cin_p)
    if skip is not None:
        S = np.zeros((Cout_p, pad_channels(skip.shape[1])), np.float16)
        S[:Cout, :skip.shape[1]] = skip[:, :, 0, 0]
        M = np.concatenate([M, S], 1)
    return M


def pack_conv(W, skip=None):
    """conv_matrix in the fragment order of csrc/mfma_tile.h, [Cout_p/32][K/16][64][8] float16."""
    M = conv_matrix(W, skip)
    return pack_matrix(M).reshape(M.shape[0] // 32, M.shape[1] // 16, 64, 8)


def weight_layout():
    """[(matrix offset, bias offset, Cout_p, K)] of LAYERS in bytes, and the buffer's size: every layer's
    packed matrix followed by its b' [Cout_p] float32, with no gaps."""
    out, at = [], 0
    for conv, _, skip in LAYERS:
        Cout, Cin, KH = _SHAPES[conv]
        K = STEM_K if Cin == 1 else KH * KH * pad_channels(Cin) + (pad_channels(_SHAPES[skip[0]][1]) if skip else 0)
        Cout_p = pad_channels(Cout)
        out.append((at, at + Cout_p * K * 2, Cout_p, K))
        at += Cout_p * K * 2 + Cout_p * 4
    return out, at


def scratch_bytes(N, H, W):
    """nof_backbone_scratch_bytes restated: three activations per level, fp16, each part rounded up to 256
    bytes. 1/2: 128, 224, 224 channels; 1/4: 224, 256, 256; 1/8: 256, 256, 256."""
    p2 = N * (H // 2) * (W // 2)
    parts = [(p2, 128), (p2, 224), (p2, 224), (p2 // 4, 224), (p2 // 4, 256), (p2 // 4, 256)] + [(p2 // 16, 256)] * 3
    return sum((p * c * 2 + 255) // 256 * 256 for p, c in parts)


class Backbone(PackedWeights):
    """ResNetFPN_8_2 with its weights folded and packed for the device.

    weights maps the reference's parameter names (conv1.weight, bn1.{weight,bias,running_mean,running_var},
    layer{1,2,3}.{0,1}.{conv1,conv2}.weight and .bn{1,2}.*, layer{2,3}.0.downsample.{0.weight,1.*},
    layer{3,2,1}_outconv.weight, layer{2,1}_outconv2.{0.weight,1.*,3.weight}) to arrays or tensors.
    Everything is one buffer (.packed, uint8) that goes to the device once: at construction when device is
    given, else at the first forward."""

    def __init__(self, weights, device=None, prefix=""):
        what = "Backbone"

        def get(key, shape):
            return self.lookup(weights, prefix, key, shape, what)

        def folded(conv, bn):
            Cout, Cin, KH = _SHAPES[conv]
            W = get(conv + ".weight", (Cout, Cin, KH, KH))
            if bn is None:
                return W.astype(np.float16), np.zeros(Cout, np.float32)
            return fold_batchnorm(W, *(get(f"{bn}.{n}", (Cout,)) for n in ("weight", "bias", "running_mean", "running_var")))

        parts = []
        for conv, bn, skip in LAYERS:
            W, b = folded(conv, bn)
            Ws = None
            if skip is not None:
                Ws, bs = folded(*skip)
                b = b + bs
            bias = np.zeros(pad_channels(W.shape[0]), np.float32)
            bias[:W.shape[0]] = b
            parts += [pack_conv(W, Ws).view(np.uint8).ravel(), bias.view(np.uint8)]
        super().__init__(np.concatenate(parts), device)
        assert self.packed.size == weight_layout()[1]
        self._scratch = self._buffers           # the name tests and scripts read
        self._pe = {}               # (device, hc, wc, temp_bug_fix) -> [hc wc, 256] f32

    @classmethod
    def from_state_dict(cls, sd, prefix=None, device=None):
        """From a checkpoint's state dict. prefix is what stands before 'conv1.weight' ('', 'backbone.',
        'matcher.backbone.'); None finds it."""
        if prefix is None:
            prefix = cls.find_prefix(sd, _PROBE, "Backbone", "a backbone")
        return cls(sd, device=device, prefix=prefix)

    def forward(self, images, position_encoding=True, temp_bug_fix=False):
        """images [N,H,W] or [N,1,H,W] (array or tensor, any float dtype, grey / 255), H and W multiples of
        8 up to 4096 -> (coarse_tokens [N, hc wc, 256] float32, fine [N,hf,wf,128] float16 channels-last,
        (hc, wc)) on the device, hc = H / 8 and hf = H / 2. The coarse tokens carry the position encoding
        (transformer.position_encoding) unless position_encoding is False: what FeatureTransformer.forward
        and FineRefiner.refine take."""
        what = "Backbone.forward"
        t = as_tensor(images)
        if not t.is_floating_point():
            raise ValueError(f"{what}: images must be a floating-point array, got {t.dtype}")
        if t.dim() == 4 and t.shape[1] == 1:
            t = t[:, 0]
        if t.dim() != 3:
            raise ValueError(f"{what}: images must be [N,H,W] or [N,1,H,W], got {tuple(t.shape)}")
        N, H, W = t.shape
        if N < 1:
            raise ValueError(f"{what}: N={N} must be at least 1")
        if H < 8 or W < 8 or H % 8 or W % 8 or H > MAX_SIDE or W > MAX_SIDE:
            raise ValueError(f"{what}: the images are {H}x{W}: both sides must be multiples of 8 in 8..{MAX_SIDE}")
        hc, wc = H // 8, W // 8
        dev = default_device(t)
        lib = _lib.lib()
        with torch.cuda.device(dev):
            x = t.to(device=dev, dtype=torch.float32).contiguous()
            w = self.device_weights(dev)
            ws = self.buffer(dev, int(lib.nof_backbone_scratch_bytes(N, H, W)))
            pe = None
            if position_encoding:
                key = (dev, hc, wc, bool(temp_bug_fix))
                if key not in self._pe:
                    self._pe[key] = _T.position_encoding(hc, wc, C_COARSE, temp_bug_fix, device=dev).contiguous()
                pe = self._pe[key]
            coarse = torch.empty((N, hc * wc, C_COARSE), dtype=torch.float32, device=dev)
            fine = torch.empty((N, H // 2, W // 2, C_FINE), dtype=torch.float16, device=dev)
            D = _lib.BackboneDesc()
            D.images, D.N, D.H, D.W = _lib.ptr(x), N, H, W
            D.weights, D.weights_bytes, D.pe = _lib.ptr(w), w.numel(), _lib.ptr(pe)
            D.coarse, D.fine = _lib.ptr(coarse), _lib.ptr(fine)
            D.scratch, D.scratch_bytes = _lib.ptr(ws), ws.numel()
            _lib.check(lib.nof_backbone(ctypes.byref(D), _lib.stream_of(x)), what)
        return coarse, fine, (hc, wc)

    __call__ = forward
