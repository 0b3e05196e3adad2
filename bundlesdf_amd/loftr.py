"""The matcher from images to refined matches: backbone -> coarse transformer -> matching head -> fine stage.

What the reference's LoFTR.forward (BundleTrack/LoFTR/src/loftr/loftr.py) does for a batch of image pairs,
chained from the stages of this package: Backbone.forward (backbone.py), FeatureTransformer.forward
(transformer.py), match_descriptors (matching.py) and FineRefiner.refine (fine.py). Torch plumbing only:
every kernel is behind one of those four. The backbone runs once per distinct frame, not once per pair.
"""
import numpy as np
import torch

from ._args import as_tensor
from .backbone import Backbone
from .fine import FineRefiner
from .matching import match_descriptors
from .transformer import FeatureTransformer

__all__ = ["Loftr"]


class Loftr:
    """.backbone, .coarse (the eight-layer FeatureTransformer) and .refiner from one checkpoint dictionary."""

    def __init__(self, backbone, coarse, refiner):
        self.backbone, self.coarse, self.refiner = backbone, coarse, refiner

    @classmethod
    def from_state_dict(cls, sd, device=None):
        """sd holds the reference's keys (backbone.*, loftr_coarse.*, fine_preprocess.*, loftr_fine.*), with
        or without a common prefix such as 'matcher.'. A missing or mis-shaped key raises ValueError naming it."""
        return cls(Backbone.from_state_dict(sd, device=device), FeatureTransformer.from_state_dict(sd, device=device),
                   FineRefiner.from_state_dict(sd, device=device))

    def match(self, images, pairs, masks=None, thr=0.2, border_rm=2, temperature=0.1):
        """images [N,H,W] or [N,1,H,W] (grey / 255), pairs [P,2] frame indices (a, b), masks [N, H/8, W/8] or
        [N, H/8 W/8] or None (0 = the coarse cell takes no part) -> the FineMatches of the P pairs."""
        what = "Loftr.match"
        p = as_tensor(pairs)
        if p.dim() != 2 or p.shape[1] != 2 or p.shape[0] < 1 or p.is_floating_point() or p.dtype == torch.bool:
            raise ValueError(f"{what}: pairs must be [P,2] integers with P >= 1, got {tuple(p.shape)} {p.dtype}")
        p = p.cpu().to(torch.int64)
        # the distinct frames, in order of their index; pairs renumbered to them
        frames, local = torch.unique(p, return_inverse=True)
        n_images = images.shape[0]
        if int(frames[0]) < 0 or int(frames[-1]) >= n_images:
            raise ValueError(f"{what}: pairs must lie in 0 .. {n_images - 1}")
        sub = images[frames.to(images.device)] if torch.is_tensor(images) else np.asarray(images)[frames.numpy()]
        tok, fine, hw = self.backbone.forward(sub)
        ia, ib = local[:, 0].to(tok.device), local[:, 1].to(tok.device)
        ma = mb = None
        if masks is not None:
            m = as_tensor(masks)
            if m.shape[0] != n_images or m[0].numel() != hw[0] * hw[1]:
                raise ValueError(f"{what}: masks must be [{n_images},{hw[0]},{hw[1]}], got {tuple(m.shape)}")
            m = (m.reshape(n_images, -1) != 0)[frames.to(m.device)].to(tok.device)
            ma, mb = m[ia], m[ib]
        da, db = self.coarse.forward(tok[ia], tok[ib], ma, mb)
        cm = match_descriptors(da, db, hw, hw, ma, mb, temperature=temperature, thr=thr, border_rm=border_rm)
        return self.refiner.refine(cm, fine, fine, da, db, frames_a=ia, frames_b=ib)
