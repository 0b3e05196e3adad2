"""Record tests/golden/feature_transformer.npz: what the reference's own LocalFeatureTransformer and
PositionEncodingSine give on the cases of tests/transformer_oracle.py.

    python tests/golden/make_feature_transformer.py /path/to/the/reference/checkout

The reference's loftr_module/transformer.py (with linear_attention.py beside it) and
utils/position_encoding.py import only torch. They are loaded by file path: a bare module with
__path__ set to their directory stands in for the package, so the package's __init__ and its einops
and yacs imports never run. Weights and inputs come from transformer_oracle's seeded generators and are
not stored. Per case the fixture (cut into shards below 1 MiB, see the end of main) holds
    a64, b64            the module's float64 outputs without masks
    a64m, b64m          its float64 outputs with the case's masks (cases that have masks)
    e16_rms, e16_max    the reference's own half-precision error: its output under
                        torch.autocast("cpu", dtype=torch.float16) WITHOUT masks minus a64 / b64, over
                        both outputs (with a masked query the reference's fp16 1 / (0 + 1e-6) is inf
                        and 0 inf is NaN, so the autocast run has no masks)
and pe_{C}_{h}x{w}_{fix}: PositionEncodingSine(C, temp_bug_fix=fix).pe[0, :, :h, :w] for both flags.
Cases with stored=False leave only e16_rms and e16_max: their float64 outputs, with and without masks,
are checked here against the oracle to 1e-9 and then dropped, and the tests take them from the oracle.

Then the mutant table (transformer_oracle.MUTANTS). For every (mutant, case) pair it prints the distance
rms(d_m) in e16_rms and alpha = <h16 - r64, d_m> / <d_m, d_m>, the component of the reference's own
half-precision error (unmasked, as e16) along the deviation d_m, and asserts |alpha| <= 0.1: a correct
half-precision evaluation stays that far from a mutant, so the GPU test's cap of 0.25 is a condition
the reference itself meets with room. Nothing of the table is stored.
Data only, none of the reference's code.
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
    T = _load(os.path.join(loftr, "loftr_module"), "transformer", "reference_loftr_module")
    PE = _load(os.path.join(loftr, "utils"), "position_encoding", "reference_loftr_utils")
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tests import transformer_oracle as O

    rec, err16 = {}, {}
    for name, c in O.CASES.items():
        w, a, b, ma, mb = O.case_data(name)
        net = T.LocalFeatureTransformer(dict(d_model=c["C"], nhead=O.H, layer_names=list(c["layers"]),
                                             attention="linear")).eval()
        missing = net.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
        ta, tb = torch.from_numpy(a), torch.from_numpy(b)
        with torch.no_grad():
            with torch.autocast("cpu", dtype=torch.float16):
                ha, hb = net(ta, tb)
            net = net.double()
            a64, b64 = net(ta.double(), tb.double())
            stored = c.get("stored", True)
            if stored:
                rec[f"{name}_a64"], rec[f"{name}_b64"] = a64.numpy(), b64.numpy()
            else:
                assert np.abs(O.flat(O.case_output(name)) - O.flat((a64.numpy(), b64.numpy()))).max() <= 1e-9, name
            if ma is not None:
                a64m, b64m = net(ta.double(), tb.double(), torch.from_numpy(ma), torch.from_numpy(mb))
                assert torch.isfinite(a64m).all() and torch.isfinite(b64m).all()
                if stored:
                    rec[f"{name}_a64m"], rec[f"{name}_b64m"] = a64m.numpy(), b64m.numpy()
                else:
                    assert np.abs(O.flat(O.case_output(name, True)) - O.flat((a64m.numpy(), b64m.numpy()))).max() <= 1e-9, name
        err = np.concatenate([(ha.double() - a64).numpy().ravel(), (hb.double() - b64).numpy().ravel()])
        assert np.isfinite(err).all()
        err16[name] = err
        rec[f"{name}_e16_rms"], rec[f"{name}_e16_max"] = np.sqrt(np.mean(err ** 2)), np.abs(err).max()
        out = np.concatenate([a64.numpy().ravel(), b64.numpy().ravel()])
        print(f"{name}: out rms {np.sqrt(np.mean(out ** 2)):.3f}  e16_rms {rec[f'{name}_e16_rms']:.3e}  "
              f"e16_max {rec[f'{name}_e16_max']:.3e}")
    print("mutant, case: rms(d_m) / e16_rms, alpha of the reference's fp16 error")
    for mutant, (cases, factor) in O.MUTANTS.items():
        for name in cases:
            d = O.mutant_delta(name, mutant)
            dist = np.sqrt(np.mean(d ** 2)) / rec[f"{name}_e16_rms"]
            alpha = O.projection(err16[name], d)
            print(f"| `{mutant}` | {name} | {dist:.1f} | {alpha:+.4f} |")
            assert abs(alpha) <= 0.1, (mutant, name, alpha)
    for C, h, w_ in O.PE_GRIDS:
        for fix in (False, True):
            rec[f"pe_{C}_{h}x{w_}_{int(fix)}"] = PE.PositionEncodingSine(C, temp_bug_fix=fix).pe[0, :, :h, :w_].numpy()
    # float64 noise does not compress and no committed file may pass 1 MiB: the [P,n,C] outputs are cut
    # into their pairs ("key@p") and dealt to shards feature_transformer.npz, feature_transformer.1.npz, ...
    # that transformer_oracle.load_golden puts together again
    parts = {}
    for k, v in rec.items():
        v = np.asarray(v)
        if v.ndim == 3 and not k.startswith("pe_"):
            parts.update({f"{k}@{p}": v[p] for p in range(v.shape[0])})
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
