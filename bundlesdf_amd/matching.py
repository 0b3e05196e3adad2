"""Descriptor matching on the device: fused dual-softmax mutual nearest neighbours.

Where the tracker's pixel matches come from. In the reference BundleSdf.find_corres gets them from
LoftrRunner.predict, whose weight-free matching head (BundleTrack/LoFTR/src/loftr/utils/
coarse_matching.py: the [N,L,S] similarity, a softmax along each axis, their product, a threshold,
a border mask and mutual nearest neighbours) works on the descriptors of any backbone. Here it is
nof_match_descriptors (csrc/match.hip, include/nof.h group 11): the similarity tiles stay in MFMA
accumulators, only row and column statistics reach memory, and every run gives the same bytes. The
header comment of csrc/match.hip is the definition; tests/match_oracle.py restates it in float64.

No CPU fallback: match_descriptors raises if libnof.so cannot run. CoarseMatches.to_pixels gives
the rows lift_matches takes, and its conf can go to ransac_pairs(conf=) as it is.
"""
import ctypes
import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._args import as_tensor, cells_to_pixels, default_device

__all__ = ["match_descriptors", "CoarseMatches", "MAX_PAIRS", "MAX_C", "TILE"]

MAX_PAIRS = 65535
MAX_C = 512
TILE = (128, 32)        # MATCH_QB, MATCH_KT of csrc/match.hip: queries of a block, keys of a staged tile


@dataclass
class CoarseMatches:
    """Tensors of one match_descriptors call (on the device it ran on)."""
    j_of_i: torch.Tensor                 # [P,L] i32: the cell of B matched to cell i of A, -1 for none
    conf: torch.Tensor                   # [P,L] f32: its confidence, 0 for none
    n_matches: torch.Tensor              # [P] i32
    hw_a: tuple                          # (h0, w0)
    hw_b: tuple                          # (h1, w1)
    row_max: Optional[torch.Tensor] = None   # [P,L] f32 (return_stats)
    row_sum: Optional[torch.Tensor] = None   # [P,L] f32
    col_max: Optional[torch.Tensor] = None   # [P,S] f32
    col_sum: Optional[torch.Tensor] = None   # [P,S] f32

    def to_pixels(self, scale=8, tf_a=None, tf_b=None):
        """(uv_a [M,2] f64, uv_b [M,2] f64, pair_start [P+1] i32, conf [M] f32) in lift_matches' layout,
        the rows ordered by (pair, i). A cell c of a grid of width w is the pixel (c % w, c // w) scale;
        with tf_a / tf_b ([3,3] or [P,3,3], the image transform the descriptors' images went through)
        it is taken through the transform's inverse (find_corres), then rounded half away from zero.
        One host read: the rows that hold a match."""
        P, L = self.j_of_i.shape
        dev = self.j_of_i.device
        pair, i = torch.nonzero(self.j_of_i >= 0, as_tuple=True)        # row-major: ordered by (pair, i)
        j = self.j_of_i[pair, i].to(torch.int64)
        counts = torch.bincount(pair, minlength=P)
        pair_start = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(counts, 0)]).to(torch.int32)
        return (cells_to_pixels(i, self.hw_a[1], pair, P, scale, tf_a, "tf_a"),
                cells_to_pixels(j, self.hw_b[1], pair, P, scale, tf_b, "tf_b"), pair_start, self.conf[pair, i])


def _descriptors(d, name):
    """(fp16 tensor [P,n,C] on the device it came from, single): float32 is rounded once with .half()."""
    t = as_tensor(d)
    if not t.is_floating_point():
        raise ValueError(f"match_descriptors: {name} must be a floating-point array, got {t.dtype}")
    if t.dim() not in (2, 3):
        raise ValueError(f"match_descriptors: {name} must be [n,C] or [P,n,C], got {tuple(t.shape)}")
    single = t.dim() == 2
    t = t[None] if single else t
    return t.half().contiguous(), single


def _grid(hw, n, name, count):
    try:
        h, w = (int(x) for x in hw)
    except (TypeError, ValueError):
        raise ValueError(f"match_descriptors: {name} must be (h, w), got {hw!r}")
    if h < 1 or w < 1 or h * w != n:
        raise ValueError(f"match_descriptors: {name}={h}x{w} does not give the {n} cells of {count}")
    return h, w


def _mask(v, shape, single, name):
    t = as_tensor(v)
    t = t[None] if (single and t.dim() == 1) else t
    if tuple(t.shape) != shape:
        raise ValueError(f"match_descriptors: {name} must be {list(shape)}, got {tuple(t.shape)}")
    return (t != 0).to(torch.uint8).contiguous()


def match_descriptors(desc_a, desc_b, hw_a, hw_b, valid_a=None, valid_b=None, *, temperature=0.1, thr=0.2, border_rm=2,
                      return_stats=False):
    """Dual-softmax mutual nearest neighbours of P descriptor pairs -> CoarseMatches.

    desc_a [P,L,C] and desc_b [P,S,C] (arrays or tensors; one [L,C] / [S,C] pair without the P axis is
    accepted and comes back as P = 1; float32 is rounded once to float16) are the descriptors of the cells of an hw_a = (h0,
    w0) and an hw_b = (h1, w1) grid, row-major; C is a multiple of 8, at most 512. valid_a [P,L] /
    valid_b [P,S] (any dtype, 0 = the cell takes no part; give both or neither) are cell masks such
    as the object mask at the descriptors' stride.

    conf(i,j) = softmax over j of sim times softmax over i of sim with sim = a_i . b_j / (C
    temperature); (i,j) is a match iff conf > thr, neither cell lies within border_rm cells of its
    grid's edge, and each is the other's best partner (ties go to the lowest index). With
    return_stats the row and column maxima and sums of exp(sim - max) come back too."""
    what = "match_descriptors"
    a, single = _descriptors(desc_a, "desc_a")
    b, single_b = _descriptors(desc_b, "desc_b")
    if single != single_b:
        raise ValueError(f"{what}: desc_a is {tuple(a.shape[1 - single:])} and desc_b {tuple(b.shape[1 - single_b:])}: "
                         "give both with the P axis or both without")
    if torch.is_tensor(desc_a) and torch.is_tensor(desc_b) and desc_a.device != desc_b.device:
        raise ValueError(f"{what}: desc_a is on {desc_a.device} and desc_b on {desc_b.device}")
    P, L, C = a.shape
    if b.shape[0] != P or b.shape[2] != C:
        raise ValueError(f"{what}: desc_a is {tuple(a.shape)} and desc_b {tuple(b.shape)}: P and C must agree")
    S = b.shape[1]
    if P < 1 or P > MAX_PAIRS:
        raise ValueError(f"{what}: {P} pairs (1 .. {MAX_PAIRS})")
    if C < 8 or C > MAX_C or C % 8:
        raise ValueError(f"{what}: C={C} must be a multiple of 8 in 8 .. {MAX_C}")
    if L < 1 or S < 1 or P * L >= 2 ** 31 or P * S >= 2 ** 31:
        raise ValueError(f"{what}: L={L} and S={S} must be at least 1 with P L and P S below 2^31")
    h0, w0 = _grid(hw_a, L, "hw_a", "desc_a")
    h1, w1 = _grid(hw_b, S, "hw_b", "desc_b")
    temperature, thr = float(temperature), float(thr)
    if not (temperature > 0 and math.isfinite(temperature)):
        raise ValueError(f"{what}: temperature={temperature} must be positive and finite")
    if not (0.0 <= thr < 1.0):
        raise ValueError(f"{what}: thr={thr} must be in [0, 1)")
    border_rm = int(border_rm)
    if border_rm < 0:
        raise ValueError(f"{what}: border_rm={border_rm} must not be negative")
    if (valid_a is None) != (valid_b is None):
        raise ValueError(f"{what}: valid_a and valid_b must be given for both sides or for neither")
    va = vb = None
    if valid_a is not None:
        va, vb = _mask(valid_a, (P, L), single, "valid_a"), _mask(valid_b, (P, S), single, "valid_b")
        for v, name in ((valid_a, "valid_a"), (valid_b, "valid_b")):
            if torch.is_tensor(v) and torch.is_tensor(desc_a) and v.device != desc_a.device:
                raise ValueError(f"{what}: {name} is on {v.device} and desc_a on {desc_a.device}")

    dev = default_device(a if a.is_cuda else b)
    lib = _lib.lib()
    i32, f32 = torch.int32, torch.float32
    with torch.cuda.device(dev):
        a, b = a.to(dev), b.to(dev)
        va, vb = (None if v is None else v.to(dev) for v in (va, vb))
        out = CoarseMatches(j_of_i=torch.empty((P, L), dtype=i32, device=dev),
                            conf=torch.empty((P, L), dtype=f32, device=dev),
                            n_matches=torch.empty(P, dtype=i32, device=dev), hw_a=(h0, w0), hw_b=(h1, w1))
        if return_stats:
            out.row_max, out.row_sum = (torch.empty((P, L), dtype=f32, device=dev) for _ in range(2))
            out.col_max, out.col_sum = (torch.empty((P, S), dtype=f32, device=dev) for _ in range(2))
        nbytes = int(lib.nof_match_workspace_bytes(P, L, S))
        ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
        D = _lib.MatchDesc()
        D.desc_a, D.desc_b, D.valid_a, D.valid_b = (_lib.ptr(x) for x in (a, b, va, vb))
        D.P, D.L, D.S, D.C, D.h0, D.w0, D.h1, D.w1 = P, L, S, C, h0, w0, h1, w1
        D.border_rm, D.temperature, D.thr = border_rm, temperature, thr
        D.workspace, D.workspace_bytes = _lib.ptr(ws), ws.numel()
        D.j_of_i, D.conf, D.n_matches = _lib.ptr(out.j_of_i), _lib.ptr(out.conf), _lib.ptr(out.n_matches)
        D.row_max, D.row_sum, D.col_max, D.col_sum = (_lib.ptr(x) for x in (out.row_max, out.row_sum, out.col_max,
                                                                            out.col_sum))
        _lib.check(lib.nof_match_descriptors(ctypes.byref(D), _lib.stream_of(a)), what)
    return out
