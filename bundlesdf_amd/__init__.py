"""bundlesdf_amd — MI355X-native neural-object-field trainer.

Drop-in for the per-step SDF/colour rendering + online optimisation loop of
BundleSDF's nerf_runner.py. Kernels live in libnof.so (HIP,
gfx950) behind the C ABI in include/nof.h; the Python modules mirror the
reference's operator/module interfaces:

  bundlesdf_amd.gridencoder   <- mycuda/torch_ngp_grid_encoder (pybind `gridencoder`)
  bundlesdf_amd.common        <- mycuda (pybind `common`)
  bundlesdf_amd.grid          <- mycuda/torch_ngp_grid_encoder/grid.py
  bundlesdf_amd.nerf_helpers  <- nerf_helpers.py
  bundlesdf_amd.nerf_runner   <- nerf_runner.py (NerfRunner)
  bundlesdf_amd.matching      <- BundleTrack/LoFTR/src/loftr/utils/coarse_matching.py (match_descriptors)
  bundlesdf_amd.transformer   <- BundleTrack/LoFTR/src/loftr/loftr_module/transformer.py, utils/position_encoding.py
  bundlesdf_amd.fine          <- BundleTrack/LoFTR/src/loftr/loftr_module/fine_preprocess.py, utils/fine_matching.py
  bundlesdf_amd.backbone      <- BundleTrack/LoFTR/src/loftr/backbone/resnet_fpn.py (ResNetFPN_8_2)
  bundlesdf_amd.loftr         <- BundleTrack/LoFTR/src/loftr/loftr.py (LoFTR.forward)
  bundlesdf_amd.pairs         <- BundleTrack/src/FeatureManager.cpp (processImagePair), Frame::updateRoi, find_corres
"""
__version__ = "0.1.0"

__all__ = ["matching", "transformer", "fine", "backbone", "loftr", "pairs"]


def __getattr__(name):
    # bundlesdf_amd.matching / .transformer / ... without an import of their own; loaded on first use so
    # that `python -m bundlesdf_amd.build` does not pay for torch
    if name in __all__:
        import importlib
        return importlib.import_module("." + name, __name__)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
