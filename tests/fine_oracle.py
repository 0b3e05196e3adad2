"""Float64 numpy restatement of the fine-level refinement's definition (the header comment of
bundlesdf_amd/csrc/fine_match.hip), with the cases, the hand-written matches and the seeded generators
that the tests and tests/golden/make_fine_match.py share. The two layers between the stages are
tests/transformer_oracle.py's. Weights are drawn again from their seeds wherever they are needed; the
inputs are stored in the fixture, because the maker scales them (see its docstring).

    fine_window[r] = fine[frame, :, stride (cell // w) + ky - 2, stride (cell % w) + kx - 2], r = 5 ky + kx,
                     zeros outside the map
    ctx    = Wd coarse[pair, cell] + b_down
    win[r] = Wm [fine_window[r] | ctx] + b_merge
    (f0, f1) = loftr_fine(win_A, win_B)
    sim[r] = f0[12] . f1[r] / sqrt(128), heat = softmax(sim), x = sum heat gx, y = sum heat gy,
    std = sqrt(max(sum heat gx^2 - x^2, 1e-10)) + sqrt(max(sum heat gy^2 - y^2, 1e-10))
    uv_B_fine = uv_B_coarse + (x, y) 2 scale_f
"""
import os

import numpy as np

from tests import transformer_oracle as TO

W = 5
WW = 25
C = 128
CC = 256
LAYERS = ("self", "cross")
SCALE_F = 2                     # image / fine map

# Matches written by hand as {pair: {i: j}}: match_descriptors' border_rm would drop the edge cells.
# "s4": every corner of both grids (A 0, 6, 35, 41; B 0, 7, 32, 39), the last cell of each, cells on each
# edge, pair 1 with no match, and A's frame 0 in pairs 0 and 2. 20 + 0 + 17 = 37 matches.
CASES = {
    "s4": dict(hw_a=(6, 7), hw_b=(5, 8), stride=4, P=3, N=3, frames_a=(0, 1, 0), frames_b=(1, 2, 0), seed=201,
               matches={0: {0: 39, 1: 7, 3: 12, 6: 0, 7: 32, 8: 9, 10: 18, 13: 8, 14: 15, 16: 20, 19: 3, 20: 36, 22: 22,
                            24: 27, 27: 31, 28: 16, 33: 11, 35: 33, 38: 25, 41: 5},
                        1: {},
                        2: {0: 0, 2: 38, 5: 13, 6: 39, 9: 1, 11: 24, 12: 30, 15: 6, 17: 19, 21: 10, 23: 35, 26: 2, 29: 14,
                            30: 21, 34: 28, 35: 32, 41: 7}}),
    "s2": dict(hw_a=(4, 5), hw_b=(5, 4), stride=2, P=2, N=2, frames_a=None, frames_b=None, seed=202,
               matches={0: {0: 19, 4: 0, 7: 9, 12: 6, 15: 16, 19: 3}, 1: {2: 5, 5: 12, 9: 19, 10: 0, 17: 10}}),
}

SHARD_BYTES = 900_000


def shard_name(i):
    return "fine_match.npz" if i == 0 else f"fine_match.{i}.npz"


def load_golden(golden_dir):
    """tests/golden/fine_match*.npz as one dict; the parts "key@n" stacked along the first axis again."""
    first = np.load(os.path.join(golden_dir, shard_name(0)))
    flat = {}
    for i in range(int(first["n_shards"])):
        with np.load(os.path.join(golden_dir, shard_name(i))) as z:
            flat.update({k: z[k] for k in z.files})
    out, parts = {}, {}
    for k, v in flat.items():
        if "@" in k:
            key, n = k.split("@")
            parts.setdefault(key, {})[int(n)] = v
        else:
            out[k] = v
    for key, d in parts.items():
        out[key] = np.concatenate([d[n] for n in range(len(d))])
    return out


def _f16(x):
    return np.asarray(x).astype(np.float16).astype(np.float32)


def case_matches(case):
    """(pair, i, j) [M] int32 ordered by (pair, i), and j_of_i [P,L] int32 with -1 for none."""
    c = CASES[case]
    L = c["hw_a"][0] * c["hw_a"][1]
    j_of_i = np.full((c["P"], L), -1, np.int32)
    for p, d in c["matches"].items():
        for i, j in d.items():
            j_of_i[p, i] = j
    pair, i = np.nonzero(j_of_i >= 0)
    return pair.astype(np.int32), i.astype(np.int32), j_of_i[pair, i], j_of_i


def make_weights(seed):
    """The reference's parameter names -> float32 arrays of fp16 values: fine_preprocess.* uniform in
    +-sqrt(6 / (fan_in + fan_out)) with biases 0.1 N(0,1), loftr_fine.* as transformer_oracle draws them."""
    rng = np.random.default_rng(seed)
    w = {}
    for name, shape in (("down_proj", (C, CC)), ("merge_feat", (C, 2 * C))):
        bound = np.sqrt(6.0 / (shape[0] + shape[1]))
        w[f"fine_preprocess.{name}.weight"] = _f16(rng.uniform(-bound, bound, size=shape))
        w[f"fine_preprocess.{name}.bias"] = _f16(0.1 * rng.standard_normal(shape[0]))
    w.update({"loftr_fine." + k: v for k, v in TO.make_weights(seed + 1, C, LAYERS).items()})
    return w


def make_inputs(case, gain):
    """(fine_a [N,128,hf0,wf0], fine_b [N,128,hf1,wf1], coarse_a [P,L,256], coarse_b [P,S,256]): gain times
    standard normal, float32 arrays of fp16 values."""
    c = CASES[case]
    rng = np.random.default_rng(c["seed"] + 1000)
    (h0, w0), (h1, w1), s = c["hw_a"], c["hw_b"], c["stride"]
    shapes = ((c["N"], C, s * h0, s * w0), (c["N"], C, s * h1, s * w1), (c["P"], h0 * w0, CC), (c["P"], h1 * w1, CC))
    return tuple(_f16(gain * rng.standard_normal(sh)) for sh in shapes)


def fine_windows(fine, frame, cell, w_grid, stride):
    """fine [N,C,hf,wf], frame [M], cell [M] -> [M,25,C]: the 5x5 window around every cell, zeros outside."""
    N, Cn, hf, wf = fine.shape
    out = np.zeros((len(cell), WW, Cn), np.float64)
    for m, (f, c) in enumerate(zip(frame, cell)):
        for r in range(WW):
            y, x = stride * (c // w_grid) + r // W - W // 2, stride * (c % w_grid) + r % W - W // 2
            if 0 <= y < hf and 0 <= x < wf:
                out[m, r] = fine[f, :, y, x]
    return out


def preprocess(w, fine, coarse, frames, pair, cell, w_grid, stride):
    """One side's FinePreprocess output [M,25,128], float64."""
    g = lambda k: w["fine_preprocess." + k].astype(np.float64)
    frame = pair if frames is None else np.asarray(frames)[pair]
    win = fine_windows(fine.astype(np.float64), frame, cell, w_grid, stride)
    ctx = coarse.astype(np.float64)[pair, cell] @ g("down_proj.weight").T + g("down_proj.bias")          # [M,128]
    both = np.concatenate([win, np.repeat(ctx[:, None], WW, 1)], 2)                                       # [M,25,256]
    return both @ g("merge_feat.weight").T + g("merge_feat.bias")


def expectation(f0, f1):
    """f0, f1 [M,25,128] -> expec [M,3] = (x, y, std)."""
    sim = np.einsum("mc,mrc->mr", f0[:, WW // 2], f1) / np.sqrt(f0.shape[2])
    e = np.exp(sim - sim.max(1, keepdims=True))
    heat = e / e.sum(1, keepdims=True)
    r = np.arange(WW)
    g = np.stack([-1.0 + 0.5 * (r % W), -1.0 + 0.5 * (r // W)], 1)                                        # [25,2] (x, y)
    mean = heat @ g
    var = heat @ g ** 2 - mean ** 2
    std = np.sqrt(np.maximum(var, 1e-10)).sum(1)
    return np.concatenate([mean, std[:, None]], 1)


def fine_pixels(j, w1, expec, scale, scale_f=SCALE_F):
    """mkpts1_f [M,2]: the coarse pixel of cell j plus (x, y) (W // 2) scale_f."""
    return np.stack([j % w1, j // w1], 1).astype(np.float64) * scale + expec[:, :2] * (W // 2) * scale_f


def refine(w, case, fine_a, fine_b, coarse_a, coarse_b):
    """The whole stage on a case -> dict(win_a, win_b, f0, f1, expec, mkpts1_f), float64."""
    c = CASES[case]
    pair, i, j, _ = case_matches(case)
    win_a = preprocess(w, fine_a, coarse_a, c["frames_a"], pair, i, c["hw_a"][1], c["stride"])
    win_b = preprocess(w, fine_b, coarse_b, c["frames_b"], pair, j, c["hw_b"][1], c["stride"])
    wt = {k[len("loftr_fine."):]: v for k, v in w.items() if k.startswith("loftr_fine.")}
    f0, f1 = TO.forward(wt, LAYERS, win_a, win_b)
    expec = expectation(f0, f1)
    return dict(win_a=win_a, win_b=win_b, f0=f0, f1=f1, expec=expec,
                mkpts1_f=fine_pixels(j, c["hw_b"][1], expec, c["stride"] * SCALE_F))
