"""Record tests/golden/backbone*.npz: what the reference's own ResNetFPN_8_2 gives on the cases of
tests/backbone_oracle.py.

    python tests/golden/make_backbone.py /path/to/the/reference/checkout

The reference's backbone/resnet_fpn.py imports only torch. It is loaded by file path: a bare module with
__path__ set to its directory stands in for the package, so the package's __init__ never runs. Weights and
inputs come from backbone_oracle's seeded generators; the weights are not stored. Per case the fixture
(cut into shards below 1 MiB, see the end of main) holds, in float64,
    images                          the input [N,H,W]
    coarse64, fine64                the module's float64 outputs [N,256,H/8,W/8], [N,128,H/2,W/2]
    {coarse,fine}_e16_{rms,max}     the reference's own half-precision error: its output under
                                    torch.autocast("cpu", dtype=torch.float16) minus the float64 one
Asserted per output: rms >= 0.1, e16_max < rms / 20, everything finite. Data only, none of the
reference's code.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(directory, module, alias):
    pkg = types.ModuleType(alias)
    pkg.__path__ = [directory]
    sys.modules[alias] = pkg
    return importlib.import_module(f"{alias}.{module}")


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    loftr = os.path.join(sys.argv[1], "BundleTrack", "LoFTR", "src", "loftr")
    R = _load(os.path.join(loftr, "backbone"), "resnet_fpn", "reference_loftr_backbone")
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tests import backbone_oracle as O

    net = R.ResNetFPN_8_2(dict(initial_dim=128, block_dims=[128, 196, 256])).eval()
    res = net.load_state_dict({k: torch.from_numpy(v) for k, v in O.make_weights().items()}, strict=False)
    assert not res.unexpected_keys and all(k.endswith("num_batches_tracked") for k in res.missing_keys), res
    net64 = R.ResNetFPN_8_2(dict(initial_dim=128, block_dims=[128, 196, 256])).eval()
    net64.load_state_dict(net.state_dict())
    net64 = net64.double()

    rec = {}
    for name in O.CASES:
        images = O.make_images(name)
        x = torch.from_numpy(images)[:, None]
        with torch.no_grad():
            with torch.autocast("cpu", dtype=torch.float16):
                half = net(x)
            full = net64(x.double())
        rec[f"{name}_images"] = images.astype(np.float64)
        for key, h, f in zip(("coarse", "fine"), half, full):
            f = f.numpy()
            err = h.double().numpy() - f
            rms = np.sqrt(np.mean(f ** 2))
            e_rms, e_max = np.sqrt(np.mean(err ** 2)), np.abs(err).max()
            assert np.isfinite(f).all() and np.isfinite(err).all()
            assert rms >= 0.1 and e_max < rms / 20, (name, key, rms, e_max)
            rec[f"{name}_{key}64"], rec[f"{name}_{key}_e16_rms"], rec[f"{name}_{key}_e16_max"] = f, e_rms, e_max
            print(f"{name} {key}: rms {rms:.3f}  e16_rms {e_rms:.3e}  e16_max {e_max:.3e}  e16_max / rms {e_max / rms:.2e}")
    # float64 noise does not compress and no committed file may pass 1 MiB: the outputs are cut into their
    # images ("key@n") and dealt to shards backbone.npz, backbone.1.npz, ... that backbone_oracle.load_golden
    # puts together again
    parts = {}
    for k, v in rec.items():
        v = np.asarray(v)
        if v.ndim == 4:
            parts.update({f"{k}@{n}": v[n] for n in range(v.shape[0])})
        else:
            parts[k] = v
    shards, room = [{}], O.SHARD_BYTES
    for k, v in parts.items():
        if v.nbytes > room and shards[-1]:
            shards.append({})
            room = O.SHARD_BYTES
        shards[-1][k] = v
        room -= v.nbytes
    shards[0]["n_shards"] = np.array(len(shards))
    for i, sh in enumerate(shards):
        out = os.path.join(HERE, O.shard_name(i))
        np.savez_compressed(out, **sh)
        print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
