"""tests/tile_oracle.py (the tile classes of a training batch from the loss definitions) on the two
committed goldens and on hand-built samples, no GPU: the classes test_gpu_production.py holds the
production step's counters, tile flags and tile lists against."""
import json
import os

import numpy as np
import pytest

from oracle import nerf_step as NS
from tests import tile_oracle as TO

# G4 and G4-amp: 96 rays x 6 tiles, every ray of type 0, so the ray-type term changes nothing here:
# 221 colour tiles with a backward, 163 sigma-only backward tiles, 192 tiles with valid samples and
# no work (rays whose depth lies beyond far with sdf >= fs_sdf), none without a valid sample and no
# colour tile without a backward
PINNED = dict(invalid=0, colour_bwd=221, sigma_bwd=163, colour_fwd=0, idle=192)


@pytest.mark.parametrize("fixture", ["train_step.npz", "train_step_amp.npz"])
def test_golden_tile_classes_are_pinned(golden_dir, fixture):
    g = np.load(os.path.join(golden_dir, fixture))
    cfg = json.loads(str(g["cfg_json"]))
    trunc = NS.truncation(cfg)
    assert (g["batch"][:, 9] == 0).all()
    sdf = g["raw"][..., 3]
    cls = TO.classify_tiles(g["batch"], g["z_vals"], sdf, g["valid"], cfg, trunc)
    assert cls.shape == (96, 6)
    assert TO.class_counts(cls) == PINNED
    assert TO.counters(cls) == dict(tiles_sigma=576, tiles_colour=221, records_colour=221, records_sigma=163)
    # no tile's class hinges on a band residual below 1e-6 of the depth (an exact zero in float32, maybe)
    assert TO.hinge_tiles(g["batch"], g["z_vals"], sdf, g["valid"], cfg, trunc) == 0
    # a tile with a backward contributes to a loss term, a tile without contributes to none: the
    # losses of the backward tiles' samples alone are the step's sdf / free-space losses
    import torch
    keep = np.repeat(np.isin(cls, (TO.COLOUR_BWD, TO.SIGMA_BWD)), TO.TILE, axis=1)
    full = NS.loss_terms_f64(torch.from_numpy(g["batch"]), torch.from_numpy(g["z_vals"]), torch.from_numpy(g["raw"]),
                             torch.from_numpy(g["valid"]), cfg, trunc)
    # the samples of every other tile are taken out of the sums by giving them an sdf no term reads (front
    # and beyond far: 2, above both thresholds; band: the zero of the residual); validity and the ray
    # weights stay as they are
    d = g["batch"][:, 6:7].astype(np.float64)
    neutral = np.where(g["z_vals"] < d - trunc, 2.0, np.where(d > cfg["far"] * cfg["sc_factor"], 2.0,
                                                               (d - g["z_vals"]) / trunc))
    raw = g["raw"].astype(np.float64).copy()
    raw[..., 3] = np.where(keep, raw[..., 3], neutral)
    part = NS.loss_terms_f64(torch.from_numpy(g["batch"]), torch.from_numpy(g["z_vals"]), torch.from_numpy(raw),
                             torch.from_numpy(g["valid"]), cfg, trunc)
    assert full["sdf_loss"] > 0 and full["fs_loss"] > 0
    np.testing.assert_allclose(part["sdf_loss"], full["sdf_loss"], rtol=1e-12)
    np.testing.assert_allclose(part["fs_loss"], full["fs_loss"], rtol=1e-12)


CFG = dict(sc_factor=1.0, near=0.1, far=2.0, neg_trunc_ratio=1.0, fs_sdf=0.001, first_frame_weight=1.0,
           fs_weight=100.0, empty_weight=0.01, trunc_weight=6000.0, rgb_weight=10.0, fs_rgb_weight=0)
TRUNC = 0.01


def _ray(depth, rtype=0.0, frame=1.0):
    b = np.zeros(12, np.float32)
    b[6], b[8], b[9] = depth, frame, rtype
    return b


def _tiles(rays, z, sdf, valid, cfg=CFG):
    return TO.classify_tiles(np.stack(rays), np.asarray(z, np.float32), np.asarray(sdf, np.float32),
                             np.asarray(valid, bool), cfg, TRUNC)


def test_every_class_from_its_definition():
    """One ray per row, two tiles each: samples in front of the band, then samples inside it."""
    front = np.linspace(0.50, 0.90, 32)
    band = np.linspace(0.992, 1.008, 32)
    z = np.concatenate([front, band])
    ones, zeros = np.ones(64, bool), np.zeros(64, bool)
    half = np.concatenate([np.zeros(32, bool), np.ones(32, bool)])
    rays = [_ray(1.0), _ray(1.0), _ray(1.0, rtype=1.0), _ray(1.0), _ray(5.0), _ray(5.0)]
    sdf = [np.full(64, 0.2),    # front samples with sdf < 1: the empty term; band samples: rgb + sdf terms
           np.full(64, 1.5),    # front samples with sdf >= 1: no term reads them
           np.full(64, 0.2),    # a type-1 ray: the band is composited, nothing carries a gradient
           np.full(64, 0.2),    # the front tile holds no valid sample
           np.full(64, -0.5),   # depth beyond far, sdf < fs_sdf: the free-space term, no compositing
           np.full(64, 0.2)]    # depth beyond far, sdf >= fs_sdf: nothing
    valid = [ones, ones, ones, half, ones, ones]
    cls = _tiles(rays, [z] * 6, sdf, valid)
    want = [[TO.SIGMA_BWD, TO.COLOUR_BWD], [TO.IDLE, TO.COLOUR_BWD], [TO.IDLE, TO.COLOUR_FWD],
            [TO.INVALID, TO.COLOUR_BWD], [TO.SIGMA_BWD, TO.SIGMA_BWD], [TO.IDLE, TO.IDLE]]
    np.testing.assert_array_equal(cls, want)
    assert TO.counters(cls) == dict(tiles_sigma=11, tiles_colour=4, records_colour=3, records_sigma=3)
    assert TO.rays_with_band_samples(np.stack(rays), np.stack([z] * 6), np.stack(valid), CFG, TRUNC) == 1
    # fs_rgb_weight > 0 reads the colour of every weighted front sample: the sigma-only front tile
    # and the idle one become colour tiles with a backward; the type-1 ray's tiles do not change
    cls_w = _tiles(rays, [z] * 6, sdf, valid, dict(CFG, fs_rgb_weight=10.0))
    np.testing.assert_array_equal(cls_w[:4], [[TO.COLOUR_BWD, TO.COLOUR_BWD], [TO.COLOUR_BWD, TO.COLOUR_BWD],
                                              [TO.IDLE, TO.COLOUR_FWD], [TO.INVALID, TO.COLOUR_BWD]])
    # a band whose every sample is invalid is not composited: the tile has no valid sample
    none = _tiles([_ray(1.0)], [z], [np.full(64, 0.2)], [~half])
    np.testing.assert_array_equal(none, [[TO.SIGMA_BWD, TO.INVALID]])


def test_hinge_tiles_counts_classes_that_rest_on_a_zero_residual():
    """A tile of samples behind the band (no term reads them) with one band sample whose residual
    z + sdf trunc - d is 1e-9 d: with the rgb term off, that residual alone gives the tile a backward."""
    z = np.full(32, 1.2)          # behind the band of d = 1
    z[7] = 1.0                    # one band sample ...
    sdf = np.zeros(32)
    sdf[7] = 1e-7                 # ... with residual 1e-9
    cfg = dict(CFG, rgb_weight=0.0)   # (the rgb term would carry the tile whatever its residual)
    batch, valid = np.stack([_ray(1.0)]), np.ones((1, 32), bool)
    assert TO.classify_tiles(batch, z[None], sdf[None], valid, cfg, TRUNC)[0, 0] == TO.COLOUR_BWD
    assert TO.classify_tiles(batch, z[None], sdf[None], valid, cfg, TRUNC, zero_rel=TO.ZERO_REL)[0, 0] == TO.COLOUR_FWD
    assert TO.hinge_tiles(batch, z[None], sdf[None], valid, cfg, TRUNC) == 1
    sdf[7] = 0.5                  # a residual of 5e-3: nothing rests on rounding
    assert TO.hinge_tiles(batch, z[None], sdf[None], valid, cfg, TRUNC) == 0
