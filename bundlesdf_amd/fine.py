"""Fine-level match refinement on the device: windows, fusion, sub-pixel expectation.

What stands between match_descriptors and lift_matches in the reference: LoFTR.forward runs
FinePreprocess (BundleTrack/LoFTR/src/loftr/loftr_module/fine_preprocess.py: a 5x5 window of the
1/2-resolution feature map around both ends of every coarse match, fused with the coarse descriptor),
loftr_fine (two linear-attention layers over each pair of windows) and FineMatching (utils/
fine_matching.py: the centre of window 0 against window 1, a softmax, the expected position) on every
coarse match, and LoftrRunner.predict returns mkpts1_f, never the 1/8-grid mkpts1_c. Here the windows
are nof_fine_windows and the expectation nof_fine_expectation (csrc/fine_match.hip, include/nof.h
group 13); the transformer between them is nof_feature_transformer on the windows in place. The
header comment of csrc/fine_match.hip is the definition; tests/fine_oracle.py restates it in float64.

No CPU fallback: FineRefiner.refine raises if libnof.so cannot run. The chain is
ft.forward -> match_descriptors -> refiner.refine -> to_pixels -> lift_matches.
"""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._args import PackedWeights, as_tensor, cells_to_pixels, default_device
from .matching import CoarseMatches
from .transformer import MAX_PAIRS, FeatureTransformer, pack_matrix

__all__ = ["FineRefiner", "FineMatches", "WINDOW", "C_FINE", "C_COARSE", "WEIGHT_BYTES", "MAX_SIDE"]

WINDOW = 5
WW = WINDOW * WINDOW
C_FINE = 128
C_COARSE = 256
WEIGHT_BYTES = 2 * C_FINE * C_COARSE * 2 + 2 * C_FINE * 4       # Wd, Wm in fp16, the two biases in f32
MAX_SIDE = 32768                                                # stride h, stride w of csrc/fine_match.hip

_KEYS = (("fine_preprocess.down_proj.weight", (C_FINE, C_COARSE)), ("fine_preprocess.down_proj.bias", (C_FINE,)),
         ("fine_preprocess.merge_feat.weight", (C_FINE, 2 * C_FINE)), ("fine_preprocess.merge_feat.bias", (C_FINE,)))
_PROBE = _KEYS[0][0]


@dataclass
class FineMatches:
    """Tensors of one FineRefiner.refine call (on the device it ran on), the rows ordered by (pair, i)."""
    pair: torch.Tensor                   # [M] i32
    i: torch.Tensor                      # [M] i32: the cell of A
    j: torch.Tensor                      # [M] i32: the cell of B
    conf: torch.Tensor                   # [M] f32: the coarse confidence
    expec: torch.Tensor                  # [M,3] f32: x, y in [-1, 1] (units of the window's half width), std
    pair_start: torch.Tensor             # [P+1] i32
    hw_a: tuple                          # (h0, w0)
    hw_b: tuple                          # (h1, w1)
    stride: int                          # fine cells per coarse cell

    def to_pixels(self, scale=8, scale_f=2, tf_a=None, tf_b=None, rounded=True):
        """(uv_a [M,2] f64, uv_b [M,2] f64, pair_start [P+1] i32, conf [M] f32) in lift_matches' layout.
        uv_a is CoarseMatches.to_pixels' bit for bit; uv_b is the coarse pixel plus (x, y) (WINDOW // 2)
        scale_f, scale_f = image / fine map, added in the descriptor image's frame before the inverse of
        tf_b (get_fine_match, then find_corres). rounded=False returns the sub-pixel values. No host read."""
        P = self.pair_start.numel() - 1
        pair = self.pair.to(torch.int64)
        offset = self.expec[:, :2].to(torch.float64) * float((WINDOW // 2) * scale_f)
        uv_a = cells_to_pixels(self.i.to(torch.int64), self.hw_a[1], pair, P, scale, tf_a, "tf_a", None, rounded)
        uv_b = cells_to_pixels(self.j.to(torch.int64), self.hw_b[1], pair, P, scale, tf_b, "tf_b", offset, rounded)
        return uv_a, uv_b, self.pair_start, self.conf


class FineRefiner(PackedWeights):
    """FinePreprocess, loftr_fine and FineMatching with their weights packed for the device.

    weights maps the reference's parameter names (fine_preprocess.down_proj.{weight,bias} [128,256],
    fine_preprocess.merge_feat.{weight,bias} [128,256], loftr_fine.layers.{i}...) to arrays or tensors.
    The two matrices are rounded once to float16 and put in the fragment order of csrc/mfma_tile.h
    (merge_feat as its fine half and its context half), the biases stay float32: one buffer (.packed,
    uint8). .transformer is the FeatureTransformer of loftr_fine."""

    def __init__(self, weights, layer_names=("self", "cross"), device=None, prefix=""):
        what = "FineRefiner"
        arr = {key: self.lookup(weights, prefix, key, shape, what) for key, shape in _KEYS}
        wd = arr[_KEYS[0][0]].astype(np.float16)
        wm = arr[_KEYS[2][0]].astype(np.float16)
        parts = [pack_matrix(wd), pack_matrix(np.ascontiguousarray(wm[:, :C_FINE])),
                 pack_matrix(np.ascontiguousarray(wm[:, C_FINE:])),
                 np.ascontiguousarray(arr[_KEYS[1][0]].astype(np.float32)),
                 np.ascontiguousarray(arr[_KEYS[3][0]].astype(np.float32))]
        packed = np.concatenate([p.view(np.uint8).ravel() for p in parts])
        assert packed.size == WEIGHT_BYTES
        try:
            self.transformer = FeatureTransformer(weights, d_model=C_FINE, layer_names=layer_names, device=device,
                                                  prefix=prefix + "loftr_fine.")
        except ValueError as e:
            raise ValueError(str(e).replace("FeatureTransformer", what, 1)) from None
        super().__init__(packed, device)

    @classmethod
    def from_state_dict(cls, sd, prefix=None, device=None, layer_names=("self", "cross")):
        """From a checkpoint's state dict. prefix is what stands before 'fine_preprocess...' and
        'loftr_fine...' ('', 'matcher.'); None finds it."""
        if prefix is None:
            prefix = cls.find_prefix(sd, _PROBE, "FineRefiner", "a fine stage")
        return cls(sd, layer_names=layer_names, device=device, prefix=prefix)

    @staticmethod
    def _fine_map(f, name, channels_last):
        """-> (tensor, channels_last) of a fine map, still where and what it was."""
        what = "FineRefiner.refine"
        t = as_tensor(f)
        if t.dim() != 4 or not t.is_floating_point():
            raise ValueError(f"{what}: {name} must be a floating-point [N,{C_FINE},hf,wf] or [N,hf,wf,{C_FINE}], got "
                             f"{tuple(t.shape)} {t.dtype}")
        if channels_last is None:
            channels_last = t.dtype == torch.float16 and t.shape[3] == C_FINE
        if t.shape[3 if channels_last else 1] != C_FINE:
            raise ValueError(f"{what}: {name} is {tuple(t.shape)}: {C_FINE} channels are needed on axis "
                             f"{3 if channels_last else 1}")
        return t, channels_last

    def refine(self, cm, fine_a, fine_b, coarse_a, coarse_b, frames_a=None, frames_b=None, chunk=8192, channels_last=None):
        """Refine every match of cm (a CoarseMatches of P pairs) -> FineMatches.

        fine_a / fine_b are the 1/2-resolution maps, [N,128,hf,wf] as a backbone gives them (any float
        dtype; converted once per call to channels-last fp16 with torch ops) or [N,hf,wf,128] fp16, which
        is used as it is (channels_last=None takes an fp16 map with 128 on its last axis for that form).
        frames_a / frames_b [P] name the map of each pair's side, so a frame in ten pairs is stored once;
        None is map p for pair p. coarse_a [P,L,256] / coarse_b [P,S,256] are the coarse transformer's
        outputs cm was made from. hf = stride h and wf = stride w on both sides. The matches are taken
        through the three stages in chunks of at most `chunk` (and at most the transformer's 32767
        problems), which bounds the window buffers and the transformer's workspace; the result does not
        depend on chunk. One host read: the match count and the largest j."""
        what = "FineRefiner.refine"
        if not isinstance(cm, CoarseMatches):
            raise ValueError(f"{what}: cm must be a CoarseMatches, got {type(cm).__name__}")
        P, L = cm.j_of_i.shape
        (h0, w0), (h1, w1) = cm.hw_a, cm.hw_b
        S = h1 * w1
        if h0 * w0 != L:
            raise ValueError(f"{what}: cm.hw_a={h0}x{w0} does not give the {L} cells of cm.j_of_i")
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"{what}: chunk={chunk} must be at least 1")
        chunk = min(chunk, MAX_PAIRS)
        fa, cl_a = self._fine_map(fine_a, "fine_a", channels_last)
        fb, cl_b = self._fine_map(fine_b, "fine_b", channels_last)
        strides = []
        for t, cl, (h, w), name in ((fa, cl_a, (h0, w0), "fine_a"), (fb, cl_b, (h1, w1), "fine_b")):
            hf, wf = (t.shape[1], t.shape[2]) if cl else (t.shape[2], t.shape[3])
            s = hf // h
            if s < 1 or hf != s * h or wf != s * w:
                raise ValueError(f"{what}: {name} is {hf}x{wf}, not a whole multiple of the coarse grid {h}x{w}")
            if hf > MAX_SIDE or wf > MAX_SIDE:
                raise ValueError(f"{what}: {name} is {hf}x{wf} (at most {MAX_SIDE} a side)")
            strides.append(s)
        if strides[0] != strides[1]:
            raise ValueError(f"{what}: fine_a has stride {strides[0]} and fine_b stride {strides[1]}")
        stride = strides[0]
        coarse = []
        for c, n, name in ((coarse_a, L, "coarse_a"), (coarse_b, S, "coarse_b")):
            t = as_tensor(c)
            if not t.is_floating_point() or tuple(t.shape) != (P, n, C_COARSE):
                raise ValueError(f"{what}: {name} must be a floating-point {[P, n, C_COARSE]}, got {tuple(t.shape)} {t.dtype}")
            coarse.append(t)
        frames = []
        for fr, t, name in ((frames_a, fa, "frames_a"), (frames_b, fb, "frames_b")):
            N = t.shape[0]
            if fr is None:
                if N != P:
                    raise ValueError(f"{what}: fine_{name[-1]} holds {N} maps for {P} pairs: give {name}")
                frames.append(None)
                continue
            v = as_tensor(fr)
            if v.dim() != 1 or v.numel() != P or v.is_floating_point() or v.dtype == torch.bool:
                raise ValueError(f"{what}: {name} must be {[P]} integers, got {tuple(v.shape)} {v.dtype}")
            if not v.is_cuda and v.numel() and (int(v.min()) < 0 or int(v.max()) >= N):
                raise ValueError(f"{what}: {name} must lie in 0 .. {N - 1}")
            frames.append(v)

        dev = default_device(cm.j_of_i)
        lib = _lib.lib()
        i32, f32, i64 = torch.int32, torch.float32, torch.int64
        with torch.cuda.device(dev):
            j_of_i = cm.j_of_i.to(dev)
            has = (j_of_i >= 0).flatten()
            counts = has.view(P, L).sum(1)
            pair_start = torch.cat([torch.zeros(1, dtype=i64, device=dev), torch.cumsum(counts, 0)]).to(i32)
            M, j_max = (int(v) for v in torch.stack([pair_start[-1].to(i64), j_of_i.max().to(i64)]).cpu())   # the host read
            if j_max >= S:
                raise ValueError(f"{what}: cm holds j={j_max} but cm.hw_b={h1}x{w1} has {S} cells")
            out = FineMatches(pair=torch.empty(M, dtype=i32, device=dev), i=torch.empty(M, dtype=i32, device=dev),
                              j=torch.empty(M, dtype=i32, device=dev), conf=torch.empty(M, dtype=f32, device=dev),
                              expec=torch.empty((M, 3), dtype=f32, device=dev), pair_start=pair_start,
                              hw_a=(h0, w0), hw_b=(h1, w1), stride=stride)
            if M == 0:
                return out
            # the rows that hold a match, ordered by (pair, i), without the host read of nonzero()
            slot = torch.where(has, torch.cumsum(has, 0) - 1, M)
            rows = torch.empty(M + 1, dtype=i64, device=dev).scatter_(0, slot, torch.arange(P * L, device=dev))[:M]
            out.pair = torch.div(rows, L, rounding_mode="floor").to(i32)
            out.i = (rows % L).to(i32)
            out.j = j_of_i.flatten()[rows].contiguous()
            out.conf = cm.conf.to(dev).flatten()[rows].to(f32)

            maps = [t.to(dev) if cl else t.to(dev).permute(0, 2, 3, 1) for t, cl in ((fa, cl_a), (fb, cl_b))]
            maps = [t.to(torch.float16).contiguous() for t in maps]
            ca, cb = (t.to(device=dev, dtype=f32).contiguous() for t in coarse)
            fr_a, fr_b = (None if v is None else v.to(device=dev, dtype=i32).contiguous() for v in frames)
            n = min(M, chunk)
            ctx = torch.empty((2 * n, C_FINE), dtype=f32, device=dev)
            win_a = torch.empty((n, WW, C_FINE), dtype=f32, device=dev)
            win_b = torch.empty((n, WW, C_FINE), dtype=f32, device=dev)
            stream = _lib.stream_of(win_a)
            for m0 in range(0, M, chunk):
                k = min(chunk, M - m0)
                pr, ii, jj = out.pair[m0:m0 + k], out.i[m0:m0 + k], out.j[m0:m0 + k]
                self._windows_into(lib, maps, (ca, cb), (fr_a, fr_b), (pr, ii, jj), P, cm.hw_a, cm.hw_b, stride, ctx, win_a,
                                   win_b, stream, what)
                self.transformer.forward_inplace(win_a[:k], win_b[:k])
                E = _lib.FineExpectationDesc()
                E.win_a, E.win_b, E.pair, E.i, E.j = (_lib.ptr(x) for x in (win_a, win_b, pr, ii, jj))
                E.M, E.P, E.L, E.S, E.expec = k, P, L, S, _lib.ptr(out.expec[m0:m0 + k])
                _lib.check(lib.nof_fine_expectation(ctypes.byref(E), stream), what)
        return out

    def _windows_into(self, lib, maps, coarse, frames, idx, P, hw_a, hw_b, stride, ctx, win_a, win_b, stream, what):
        """nof_fine_windows on the matches idx = (pair, i, j) into the first rows of ctx, win_a and win_b."""
        D = _lib.FineWindowsDesc()
        D.fine_a, D.fine_b, D.coarse_a, D.coarse_b = (_lib.ptr(x) for x in (maps[0], maps[1], coarse[0], coarse[1]))
        D.frames_a, D.frames_b = _lib.ptr(frames[0]), _lib.ptr(frames[1])
        D.pair, D.i, D.j = (_lib.ptr(x) for x in idx)
        D.M, D.P, D.N_a, D.N_b = idx[0].numel(), P, maps[0].shape[0], maps[1].shape[0]
        D.h0, D.w0, D.h1, D.w1, D.stride = hw_a[0], hw_a[1], hw_b[0], hw_b[1], stride
        w = self.device_weights(win_a.device)
        D.weights, D.weights_bytes = _lib.ptr(w), w.numel()
        D.context, D.win_a, D.win_b = _lib.ptr(ctx), _lib.ptr(win_a), _lib.ptr(win_b)
        _lib.check(lib.nof_fine_windows(ctypes.byref(D), stream), what)

    def windows(self, pair, i, j, fine_a, fine_b, coarse_a, coarse_b, hw_a, hw_b, frames_a=None, frames_b=None):
        """The first stage alone, for tests and tools: (win_a, win_b) [M,25,128] f32 of the matches (pair,
        i, j) [M] in one call. fine_* are channels-last fp16 device tensors [N,hf,wf,128], coarse_* f32
        device tensors [P,n,256]; nothing is validated here beyond what the entry point checks."""
        what = "FineRefiner.windows"
        dev = fine_a.device
        i32, f32 = torch.int32, torch.float32
        lib = _lib.lib()
        with torch.cuda.device(dev):
            idx = tuple(torch.as_tensor(v).to(device=dev, dtype=i32).contiguous() for v in (pair, i, j))
            M = idx[0].numel()
            frames = tuple(None if v is None else torch.as_tensor(v).to(device=dev, dtype=i32).contiguous()
                           for v in (frames_a, frames_b))
            ctx = torch.empty((2 * max(M, 1), C_FINE), dtype=f32, device=dev)
            win_a = torch.empty((M, WW, C_FINE), dtype=f32, device=dev)
            win_b = torch.empty((M, WW, C_FINE), dtype=f32, device=dev)
            if M:
                self._windows_into(lib, (fine_a, fine_b), (coarse_a, coarse_b), frames, idx, coarse_a.shape[0], hw_a, hw_b,
                                   fine_a.shape[1] // hw_a[0], ctx, win_a, win_b, _lib.stream_of(win_a), what)
        return win_a, win_b
