"""Float64 numpy restatement of descriptor matching (bundlesdf_amd/csrc/match.hip, include/nof.h group 11).

Definition. For P pairs, desc_a [P,L,C] and desc_b [P,S,C] in float16, grids (h0,w0) and (h1,w1) with
L = h0 w0 and S = h1 w1, optional cell masks valid_a [P,L] and valid_b [P,S]:

  sim(i,j)  = (sum_k a_ik b_jk) * 1/(C temperature); -inf where valid_a[i] or valid_b[j] is 0.
  conf(i,j) = exp(sim - rowmax_i) / rowsum_i * exp(sim - colmax_j) / colsum_j, the row statistics over
              j and the column statistics over i (rowsum_i = sum_j exp(sim(i,j) - rowmax_i)). A row or
              column with no valid partner has max -inf, sum 0 and conf 0 everywhere.
  (i,j) is a match iff conf(i,j) > thr, neither cell lies within border_rm cells of its grid's edge,
              j is the lowest index attaining the maximum of row i and i is the lowest index attaining
              the maximum of column j.

Everything here is float64 on the float16 inputs widened exactly; temperature and thr are taken as the
float32 numbers the C ABI carries. The sum over k runs in index order for every (i,j) alike (einsum
without BLAS), so equal descriptor rows give equal bits and ties are real ties.
"""
import numpy as np


def _f16(d):
    d = np.asarray(d)
    if d.dtype != np.float16:
        d = d.astype(np.float32).astype(np.float16)      # rounded once, as .half() does
    return d.astype(np.float64)


def inside(n_h, n_w, border):
    """[n_h n_w] bool: the cells further than `border` cells from every edge of the grid."""
    y, x = np.divmod(np.arange(n_h * n_w), n_w)
    return (x >= border) & (x < n_w - border) & (y >= border) & (y < n_h - border)


def similarity(desc_a, desc_b, valid_a=None, valid_b=None, temperature=0.1):
    """(sim [P,L,S] f64 with -inf at masked entries, abs_dot [P,L,S] = sum_k |a_ik b_jk|)."""
    a, b = _f16(desc_a), _f16(desc_b)
    C = a.shape[-1]
    scale = 1.0 / (C * float(np.float32(temperature)))
    dot = np.einsum("plc,psc->pls", a, b, optimize=False)
    abs_dot = np.einsum("plc,psc->pls", np.abs(a), np.abs(b), optimize=False)
    sim = dot * scale
    if valid_a is not None:
        ok = (np.asarray(valid_a) != 0)[:, :, None] & (np.asarray(valid_b) != 0)[:, None, :]
        sim = np.where(ok, sim, -np.inf)
    return sim, abs_dot


def softmax_stats(sim, axis):
    """(max, sum of exp(sim - max)) along axis; (-inf, 0) where nothing is valid."""
    m = sim.max(axis)
    safe = np.where(np.isfinite(m), m, 0.0)
    e = np.exp(sim - np.expand_dims(safe, axis))          # exp(-inf) = 0 at masked entries
    return m, e.sum(axis)


def confidence(sim):
    """conf [P,L,S] and the four statistics."""
    row_max, row_sum = softmax_stats(sim, 2)
    col_max, col_sum = softmax_stats(sim, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.exp(sim - np.where(np.isfinite(row_max), row_max, 0.0)[:, :, None]) / row_sum[:, :, None]
        c = np.exp(sim - np.where(np.isfinite(col_max), col_max, 0.0)[:, None, :]) / col_sum[:, None, :]
    r = np.where(row_sum[:, :, None] > 0, r, 0.0)
    c = np.where(col_sum[:, None, :] > 0, c, 0.0)
    return r * c, dict(row_max=row_max, row_sum=row_sum, col_max=col_max, col_sum=col_sum)


def match(desc_a, desc_b, hw_a, hw_b, valid_a=None, valid_b=None, temperature=0.1, thr=0.2, border_rm=2):
    """dict: j_of_i [P,L] i32 (-1 none), conf [P,L] f64 (0 none), n_matches [P] i32, the statistics, and the
    matrices sim / conf_matrix / abs_dot the tests derive their bounds from."""
    desc_a, desc_b = np.asarray(desc_a), np.asarray(desc_b)
    if desc_a.ndim == 2:
        desc_a, desc_b = desc_a[None], desc_b[None]
        if valid_a is not None:
            valid_a, valid_b = np.asarray(valid_a).reshape(1, -1), np.asarray(valid_b).reshape(1, -1)
    P, L, _ = desc_a.shape
    S = desc_b.shape[1]
    (h0, w0), (h1, w1) = hw_a, hw_b
    assert h0 * w0 == L and h1 * w1 == S
    sim, abs_dot = similarity(desc_a, desc_b, valid_a, valid_b, temperature)
    conf, stats = confidence(sim)
    row_best = conf.argmax(2)                             # numpy's argmax: the lowest index of the maximum
    col_best = conf.argmax(1)
    pi = np.arange(P)[:, None]
    ii = np.arange(L)[None, :]
    c = conf[pi, ii, row_best]
    hit = (c > float(np.float32(thr))) & (col_best[pi, row_best] == ii) & inside(h0, w0, border_rm)[None, :] & \
        inside(h1, w1, border_rm)[row_best]
    out = dict(j_of_i=np.where(hit, row_best, -1).astype(np.int32), conf=np.where(hit, c, 0.0),
               n_matches=hit.sum(1).astype(np.int32), row_best=row_best, col_best=col_best, sim=sim, conf_matrix=conf,
               abs_dot=abs_dot)
    out.update(stats)
    return out


def to_pixels(j_of_i, conf, hw_a, hw_b, scale=8, tf_a=None, tf_b=None):
    """(uv_a [M,2], uv_b [M,2], pair_start [P+1], conf [M]) of CoarseMatches.to_pixels, rows by (pair, i)."""
    j_of_i = np.asarray(j_of_i)
    P = j_of_i.shape[0]
    pair, i = np.nonzero(j_of_i >= 0)
    j = j_of_i[pair, i]

    def pixels(cell, w, tf):
        xy = np.stack([cell % w, cell // w], 1).astype(np.float64) * float(scale)
        if tf is not None:
            T = np.broadcast_to(np.asarray(tf, np.float64), (P, 3, 3))
            Ti = np.linalg.inv(T)[pair]
            q = (Ti[:, :, 0] * xy[:, 0:1] + Ti[:, :, 1] * xy[:, 1:2]) + Ti[:, :, 2]
            xy = q[:, :2] / q[:, 2:3]
        return np.sign(xy) * np.floor(np.abs(xy) + 0.5)       # C round(): halves away from zero

    pair_start = np.concatenate([[0], np.cumsum(np.bincount(pair, minlength=P))]).astype(np.int32)
    return pixels(i, hw_a[1], tf_a), pixels(j, hw_b[1], tf_b), pair_start, np.asarray(conf)[pair, i]


def planted(P, hw_a, hw_b, C, seed, masks=False, noise=0.05, sigma=1.4):
    """Planted descriptors: a random subset of B's rows is a permuted copy of A's rows plus `noise`
    (relative) noise; the rest of both is random. -> desc_a, desc_b (float16), valid_a, valid_b (uint8 or
    None), truth [P,L] (the row of B that copies row i, -1 for none)."""
    rng = np.random.default_rng(seed)
    L, S = hw_a[0] * hw_a[1], hw_b[0] * hw_b[1]
    a = rng.normal(0.0, sigma, (P, L, C))
    b = rng.normal(0.0, sigma, (P, S, C))
    truth = np.full((P, L), -1, np.int64)
    n = max(1, min(L, S) * 2 // 3)
    for p in range(P):
        src, dst = rng.permutation(L)[:n], rng.permutation(S)[:n]
        b[p, dst] = a[p, src] * (1.0 + noise * rng.normal(size=(n, C)))
        truth[p, src] = dst
    va = vb = None
    if masks:
        va = (rng.uniform(size=(P, L)) < 0.8).astype(np.uint8)
        vb = (rng.uniform(size=(P, S)) < 0.8).astype(np.uint8)
    return a.astype(np.float16), b.astype(np.float16), va, vb, truth
