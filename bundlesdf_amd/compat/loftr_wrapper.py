"""The reference's loftr_wrapper.LoftrRunner on the device stages of this package (bundlesdf_amd.loftr.Loftr):
predict(rgbAs, rgbBs) as BundleSdf.find_corres calls it. The checkpoint is whatever the caller hands over, a
state dict or the path of one; nothing else is opened."""
import numpy as np
import torch

from bundlesdf_amd.loftr import Loftr

__all__ = ["LoftrRunner", "to_grey", "pack_corres"]


def to_grey(rgbs):
    """(N,H,W,C) uint8 or float, C = 3 or 1 -> [N,H,W] float32 in 0..1: 0.2989 R + 0.587 G + 0.114 B when
    C = 3 (torchvision's rgb_to_grayscale, as the reference), then / 255."""
    a = np.asarray(rgbs)
    if a.ndim != 4 or a.shape[3] not in (1, 3):
        raise ValueError(f"LoftrRunner.predict: images must be (N,H,W,3) or (N,H,W,1), got {a.shape}")
    a = a.astype(np.float32)
    grey = 0.2989 * a[..., 0] + 0.587 * a[..., 1] + 0.114 * a[..., 2] if a.shape[3] == 3 else a[..., 0]
    return (grey / 255.0).astype(np.float32)


def pack_corres(fm):
    """FineMatches of P pairs -> a list of P float32 arrays [m_p, 5] = (u0, v0, u1, v1, conf), sub-pixel."""
    uv_a, uv_b, pair_start, conf = fm.to_pixels(rounded=False)
    rows = torch.cat([uv_a.double(), uv_b.double(), conf.double()[:, None]], 1).cpu().numpy().astype(np.float32)
    start = pair_start.cpu().numpy()
    return [rows[start[p]:start[p + 1]] for p in range(len(start) - 1)]


class LoftrRunner:
    def __init__(self, state_dict_or_path, device=None, thr=0.2):
        sd = state_dict_or_path
        if not isinstance(sd, dict):
            sd = torch.load(sd, map_location="cpu")
        self.matcher = Loftr.from_state_dict(sd.get("state_dict", sd), device=device)
        self.thr = thr

    @torch.no_grad()
    def predict(self, rgbAs, rgbBs):
        """rgbAs, rgbBs (N,H,W,C): image n of A against image n of B -> list of N arrays [m_n, 5]."""
        a, b = to_grey(rgbAs), to_grey(rgbBs)
        if a.shape != b.shape:
            raise ValueError(f"LoftrRunner.predict: rgbAs is {a.shape} and rgbBs {b.shape}")
        n = a.shape[0]
        pairs = np.stack([np.arange(n), n + np.arange(n)], 1)
        return pack_corres(self.matcher.match(np.concatenate([a, b]), pairs, thr=self.thr))
