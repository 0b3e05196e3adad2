"""Which 32-sample tiles of a training batch carry work, from the loss definitions alone (test
infrastructure). The fused step runs the sigma net on every tile that holds a valid sample, the
colour net on the tiles some colour term reads, and the backward on the tiles some loss gradient
reaches; FusedStep.tile_counters() reports how many of each it ran. This module derives the same
numbers in float64 from an oracle step's per-sample records (z_vals, raw[..., 3], valid), the
batch (depth, ray type) and the step's truncation, following the loss terms as
oracle/nerf_step.py:loss_terms_f64 restates them (train_loop nerf_runner.py:687-731, raw2outputs
:1131-1168, get_sdf_loss nerf_helpers.py:367-399):

  a sample's colour is read   when its compositing weight is non-zero (the band |z - d| of a ray whose depth
                              is not beyond far, valid sample), or — cfg fs_rgb_weight > 0 — when it is a
                              front sample with a non-zero sample weight (fs_rgb_loss);
  its sdf carries a gradient  when its sample weight is non-zero and one of the three sdf terms is:
                              free space (depth beyond far, sdf < fs_sdf), empty (front, sdf < 1) or the
                              band's sdf term (z + sdf trunc - d != 0);
  the sample weight           is non-zero on valid samples of rays of type 0 (a ray of another type has ray
                              weight 0: neither rgb_loss nor any sample term reaches it).

A tile's class follows from its 32 samples: no valid sample; colour read and a gradient (the rgb
term's included); a gradient into the sdf only; colour read without any gradient (a ray of type
!= 0 inside the band: rgb_map is composited for every ray); valid samples and nothing else."""
import numpy as np

TILE = 32
INVALID, COLOUR_BWD, SIGMA_BWD, COLOUR_FWD, IDLE = range(5)
CLASS_NAMES = ("invalid", "colour_bwd", "sigma_bwd", "colour_fwd", "idle")
# a band sample whose residual z + sdf trunc - d is below this fraction of the depth could read as an
# exact zero in another implementation's float32 (hinge_tiles)
ZERO_REL = 1e-6


def _f64(a):
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, np.float64)


def sample_terms(batch, z, sdf, valid, cfg, trunc, zero_rel=0.0):
    """Per-sample booleans [R,S]: (colour read, sdf gradient, valid). zero_rel > 0 treats a band
    residual |z + sdf trunc - d| < zero_rel d as zero."""
    batch, z, sdf = _f64(batch), _f64(z), _f64(sdf)
    valid = np.asarray(valid.detach().cpu().numpy() if hasattr(valid, "detach") else valid).astype(bool)
    sc = cfg["sc_factor"]
    near, far = cfg["near"] * sc, cfg["far"] * sc
    ntr = cfg["neg_trunc_ratio"]
    d = batch[:, 6:7]
    rtype = batch[:, 9:10]
    # raw2outputs: weights are zero on rays whose depth is beyond far and outside the band
    band = (z - d <= trunc * ntr) & (z - d >= -trunc)
    composited = band & ~(d > far) & valid
    # train_loop: ray weight (valid ray of type 0; first_frame_weight scales it), sample weight
    rw = (valid.any(-1, keepdims=True) & (rtype == 0)) * np.where(batch[:, 8:9] == 0, cfg["first_frame_weight"], 1.0)
    sw = np.where(rtype == 1, 0.0, rw * valid)
    weighted = sw != 0
    front = z < d - trunc
    back = z > d + trunc * ntr
    vdm = (d >= near) & (d <= far)
    fsm = (d > far) & (sdf < cfg["fs_sdf"])
    em = front & (d <= far) & (sdf < 1)
    resid = (z + sdf * trunc - d) * (~front & ~back & vdm)
    g_fs = fsm & (sdf - cfg["fs_sdf"] != 0) & (cfg["fs_weight"] != 0)
    g_em = em & (cfg["fs_weight"] * cfg["empty_weight"] != 0)
    g_sdf = (np.abs(resid) > zero_rel * np.abs(d)) & (resid != 0) & (cfg["trunc_weight"] != 0)
    grad = weighted & (g_fs | g_em | g_sdf)
    fs_rgb = (float(cfg.get("fs_rgb_weight", 0) or 0) > 0) & front & weighted
    rgb_grad = composited & (rw != 0) & (cfg["rgb_weight"] != 0)
    return composited | fs_rgb, grad | rgb_grad | fs_rgb, valid


def classify_tiles(batch, z, sdf, valid, cfg, trunc, zero_rel=0.0):
    """Class of every tile, int [R, S / 32] (INVALID .. IDLE)."""
    colour, grad, valid = sample_terms(batch, z, sdf, valid, cfg, trunc, zero_rel)
    R, S = valid.shape
    assert S % TILE == 0
    t = lambda m: m.reshape(R, S // TILE, TILE).any(-1)   # noqa: E731
    colour, grad, valid = t(colour), t(grad), t(valid)
    cls = np.full(valid.shape, IDLE, np.int64)
    cls[colour & grad] = COLOUR_BWD
    cls[~colour & grad] = SIGMA_BWD
    cls[colour & ~grad] = COLOUR_FWD
    cls[~valid] = INVALID
    return cls


def class_counts(cls):
    return {name: int((cls == k).sum()) for k, name in enumerate(CLASS_NAMES)}


def counters(cls):
    """FusedStep.tile_counters() of a step that ran exactly the classified work."""
    n = class_counts(cls)
    return {"tiles_sigma": n["colour_bwd"] + n["sigma_bwd"] + n["colour_fwd"] + n["idle"],
            "tiles_colour": n["colour_bwd"] + n["colour_fwd"],
            "records_colour": n["colour_bwd"], "records_sigma": n["sigma_bwd"]}


def hinge_tiles(batch, z, sdf, valid, cfg, trunc):
    """Tiles whose class changes when band residuals below ZERO_REL of the depth count as zero: the
    class of such a tile hinges on samples another float32 implementation may see as exact zeros."""
    a = classify_tiles(batch, z, sdf, valid, cfg, trunc)
    b = classify_tiles(batch, z, sdf, valid, cfg, trunc, zero_rel=ZERO_REL)
    return int((a != b).sum())


def rays_with_band_samples(batch, z, valid, cfg, trunc, rtype_nonzero=True):
    """Rays of type != 0 (or, rtype_nonzero False, of type 0) that hold a composited sample."""
    batch = _f64(batch)
    cfg0 = dict(cfg, fs_rgb_weight=0)
    colour, _, _ = sample_terms(batch, z, np.zeros_like(_f64(z)), valid, cfg0, trunc)
    sel = (batch[:, 9] != 0) if rtype_nonzero else (batch[:, 9] == 0)
    return int((colour.any(-1) & sel).sum())
