"""Record tests/golden/coarse_match.npz: what the reference's own matching head gives on small inputs.

    python tests/golden/make_coarse_match.py /path/to/the/reference/checkout

The reference's BundleTrack/LoFTR/src/loftr/utils/coarse_matching.py is loaded by file path (it imports
only torch and einops; importing the package would need yacs and kornia) and CoarseMatching.forward
runs in float64 on float16-valued descriptors without masks, in eval mode, with dual_softmax, thr 0.2,
border_rm 2 and temperature 0.1. The fixture holds the inputs and the module's b_ids, i_ids, j_ids and
mconf: data only, none of the reference's code.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
HW_A, HW_B, C, P = (12, 14), (11, 13), 24, 3


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    path = os.path.join(sys.argv[1], "BundleTrack", "LoFTR", "src", "loftr", "utils", "coarse_matching.py")
    spec = importlib.util.spec_from_file_location("reference_coarse_matching", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tests import match_oracle as O

    head = mod.CoarseMatching(dict(thr=0.2, border_rm=2, train_coarse_percent=0.4, train_pad_num_gt_min=200,
                                   match_type="dual_softmax", dsmax_temperature=0.1)).eval()
    a, b, _, _, _ = O.planted(P, HW_A, HW_B, C, seed=2024)
    data = dict(hw0_i=(HW_A[0] * 8, HW_A[1] * 8), hw1_i=(HW_B[0] * 8, HW_B[1] * 8), hw0_c=HW_A, hw1_c=HW_B)
    with torch.no_grad():
        head(torch.from_numpy(a.astype(np.float64)), torch.from_numpy(b.astype(np.float64)), data)
    out = os.path.join(HERE, "coarse_match.npz")
    np.savez_compressed(out, desc_a=a, desc_b=b, hw_a=np.array(HW_A), hw_b=np.array(HW_B), temperature=0.1, thr=0.2,
                        border_rm=2, b_ids=data["b_ids"].numpy(), i_ids=data["i_ids"].numpy(), j_ids=data["j_ids"].numpy(),
                        mconf=data["mconf"].numpy())
    print(out, "matches:", len(data["b_ids"]))


if __name__ == "__main__":
    main()
