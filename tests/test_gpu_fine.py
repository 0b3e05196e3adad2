"""GPU: bundlesdf_amd.fine (csrc/fine_match.hip, include/nof.h group 13) against the reference's
FinePreprocess, loftr_fine and FineMatching.

The yardstick is tests/golden/fine_match*.npz: the reference modules' float64 outputs on the cases of
tests/fine_oracle.py and their own half-precision error e16 (output under fp16 autocast minus float64).
As tests/test_gpu_transformer.py argues, the kernels round to fp16 at other points than autocast does,
so the two errors are independent draws of one size: the bound is 2 x e16, rms and max, for the windows,
for expec (through all three stages) and for the sub-pixel coordinates. A wrong axis order, window
offset or centre row is off by far more (tests/test_fine_cpu.py shows by how much). Everything else
here is compared bit for bit."""
import numpy as np
import pytest
import torch

from tests import fine_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return O.load_golden(golden_dir)


_RUNS = {}


def _coarse(case, dev, keep=None):
    """The case's hand-written matches as a CoarseMatches on dev; keep = n leaves the first n of them."""
    from bundlesdf_amd.matching import CoarseMatches
    c = O.CASES[case]
    pair, i, _, j_of_i = O.case_matches(case)
    j_of_i = j_of_i.copy()
    if keep is not None:
        j_of_i[pair[keep:], i[keep:]] = -1
    conf = np.where(j_of_i >= 0, np.random.default_rng(9).uniform(0.2, 1.0, j_of_i.shape), 0.0).astype(np.float32)
    return CoarseMatches(j_of_i=torch.from_numpy(j_of_i).to(dev), conf=torch.from_numpy(conf).to(dev),
                         n_matches=torch.from_numpy((j_of_i >= 0).sum(1).astype(np.int32)).to(dev), hw_a=c["hw_a"],
                         hw_b=c["hw_b"])


def _run(case, dev, golden):
    """(refiner, keyword arguments of refine, FineMatches of the whole case), once per case."""
    from bundlesdf_amd.fine import FineRefiner
    if case not in _RUNS:
        c = O.CASES[case]
        r = FineRefiner.from_state_dict(O.make_weights(c["seed"]), device=dev)
        kw = {k: torch.from_numpy(golden[f"{case}_{k}"]).float().to(dev) for k in ("fine_a", "fine_b", "coarse_a", "coarse_b")}
        kw.update(frames_a=c["frames_a"], frames_b=c["frames_b"])
        fm = r.refine(_coarse(case, dev), **kw)
        torch.cuda.synchronize()
        _RUNS[case] = (r, kw, fm)
    return _RUNS[case]


def _ratios(label, err, e_rms, e_max):
    rms, mx = float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())
    print(f"{label}: rms {rms:.3e} = {rms / e_rms:.2f} e16_rms, max {mx:.3e} = {mx / e_max:.2f} e16_max")
    return rms, mx


@pytest.mark.parametrize("case", list(O.CASES))
def test_windows_against_the_reference_module(cuda_device, golden, case):
    c = O.CASES[case]
    r, kw, _ = _run(case, cuda_device, golden)
    pair, i, j, _ = O.case_matches(case)
    cl = lambda t: t.permute(0, 2, 3, 1).half().contiguous()
    wa, wb = r.windows(pair, i, j, cl(kw["fine_a"]), cl(kw["fine_b"]), kw["coarse_a"], kw["coarse_b"], c["hw_a"], c["hw_b"],
                       c["frames_a"], c["frames_b"])
    assert wa.dtype == torch.float32 and tuple(wa.shape) == tuple(wb.shape) == (len(pair), 25, 128)
    assert torch.isfinite(wa).all() and torch.isfinite(wb).all()
    err = np.concatenate([(wa.double().cpu().numpy() - golden[f"{case}_win_a"]).ravel(),
                          (wb.double().cpu().numpy() - golden[f"{case}_win_b"]).ravel()])
    e_rms, e_max = float(golden[f"{case}_win_e16_rms"]), float(golden[f"{case}_win_e16_max"])
    rms, mx = _ratios(f"{case} windows", err, e_rms, e_max)
    assert rms <= 2 * e_rms, (case, rms, e_rms)
    assert mx <= 2 * e_max, (case, mx, e_max)


@pytest.mark.parametrize("case", list(O.CASES))
def test_expectation_and_pixels_against_the_reference_modules(cuda_device, golden, case):
    c = O.CASES[case]
    _, _, fm = _run(case, cuda_device, golden)
    pair, i, j, j_of_i = O.case_matches(case)
    assert fm.expec.dtype == torch.float32 and tuple(fm.expec.shape) == (len(pair), 3)
    for got, want in ((fm.pair, pair), (fm.i, i), (fm.j, j)):
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(fm.pair_start.cpu().numpy(), np.concatenate([[0], np.cumsum((j_of_i >= 0).sum(1))]))
    assert fm.stride == c["stride"] and fm.hw_a == c["hw_a"] and fm.hw_b == c["hw_b"]
    cm = _coarse(case, cuda_device)
    assert torch.equal(fm.conf, cm.conf[fm.pair.long(), fm.i.long()])
    for key, got in (("expec_f", fm.expec.double().cpu().numpy()),
                     ("mkpts1_f", fm.to_pixels(scale=c["stride"] * O.SCALE_F, rounded=False)[1].cpu().numpy())):
        assert np.isfinite(got).all()
        e_rms, e_max = float(golden[f"{case}_{key}_e16_rms"]), float(golden[f"{case}_{key}_e16_max"])
        rms, mx = _ratios(f"{case} {key}", got - golden[f"{case}_{key}"], e_rms, e_max)
        assert rms <= 2 * e_rms, (case, key, rms, e_rms)
        assert mx <= 2 * e_max, (case, key, mx, e_max)


def test_same_bytes_on_every_call_and_for_every_chunking(cuda_device, golden):
    r, kw, fm = _run("s4", cuda_device, golden)
    cm = _coarse("s4", cuda_device)
    for extra in (dict(), dict(chunk=3), dict(chunk=36), dict(chunk=10 ** 9)):
        again = r.refine(cm, **kw, **extra)
        assert torch.equal(again.expec, fm.expec), extra
        assert torch.equal(again.j, fm.j) and torch.equal(again.conf, fm.conf) and torch.equal(again.pair_start, fm.pair_start)


def test_every_pair_on_its_own(cuda_device, golden):
    from bundlesdf_amd.matching import CoarseMatches
    r, kw, fm = _run("s4", cuda_device, golden)
    cm = _coarse("s4", cuda_device)
    c = O.CASES["s4"]
    ps = fm.pair_start.cpu().numpy()
    for p in range(c["P"]):
        one = CoarseMatches(j_of_i=cm.j_of_i[p:p + 1], conf=cm.conf[p:p + 1], n_matches=cm.n_matches[p:p + 1], hw_a=cm.hw_a,
                            hw_b=cm.hw_b)
        got = r.refine(one, kw["fine_a"], kw["fine_b"], kw["coarse_a"][p:p + 1], kw["coarse_b"][p:p + 1],
                       frames_a=c["frames_a"][p:p + 1], frames_b=c["frames_b"][p:p + 1])
        assert tuple(got.expec.shape) == (ps[p + 1] - ps[p], 3), p        # pair 1 has no match: empty, no launch
        assert torch.equal(got.expec, fm.expec[ps[p]:ps[p + 1]]), p
        assert got.pair_start.cpu().tolist() == [0, ps[p + 1] - ps[p]]


def test_channels_first_float32_equals_channels_last_float16(cuda_device, golden):
    r, kw, fm = _run("s4", cuda_device, golden)
    cm = _coarse("s4", cuda_device)
    cl = dict(kw, fine_a=kw["fine_a"].permute(0, 2, 3, 1).half().contiguous(),
              fine_b=kw["fine_b"].permute(0, 2, 3, 1).half().contiguous())
    assert torch.equal(r.refine(cm, **cl).expec, fm.expec)
    assert torch.equal(r.refine(cm, **cl, channels_last=True).expec, fm.expec)
    half = dict(kw, fine_a=kw["fine_a"].half(), fine_b=kw["fine_b"].half())     # the maps hold fp16 values
    assert torch.equal(r.refine(cm, **half).expec, fm.expec)
    host = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in kw.items()}
    got = r.refine(cm, **host)
    assert got.expec.is_cuda and torch.equal(got.expec, fm.expec)


@pytest.mark.parametrize("n", [0, 1, 4, 5, 37])
def test_match_counts_around_a_block_of_four_waves(cuda_device, golden, n):
    r, kw, fm = _run("s4", cuda_device, golden)
    got = r.refine(_coarse("s4", cuda_device, keep=n), **kw)
    assert tuple(got.expec.shape) == (n, 3) and tuple(got.pair.shape) == tuple(got.conf.shape) == (n,)
    assert int(got.pair_start[-1]) == n and got.pair_start.numel() == 4
    assert torch.equal(got.expec, fm.expec[:n]) and torch.equal(got.j, fm.j[:n])
    uv_a, uv_b, ps, conf = got.to_pixels()
    assert tuple(uv_a.shape) == tuple(uv_b.shape) == (n, 2) and uv_a.dtype == torch.float64


def test_out_of_range_rows_are_written_as_zeros(cuda_device, golden):
    """A pair, cell or frame outside its range gives a zero window and a zero expec row, and leaves the
    other rows what they were."""
    c = O.CASES["s4"]
    r, kw, fm = _run("s4", cuda_device, golden)
    pair, i, j, _ = (x.copy() if isinstance(x, np.ndarray) else x for x in O.case_matches("s4"))
    cl = lambda t: t.permute(0, 2, 3, 1).half().contiguous()
    args = (cl(kw["fine_a"]), cl(kw["fine_b"]), kw["coarse_a"], kw["coarse_b"], c["hw_a"], c["hw_b"])
    good = r.windows(pair, i, j, *args, c["frames_a"], c["frames_b"])
    pair[3], i[5], j[7], j[9] = 3, 42, 40, -1
    wa, wb = r.windows(pair, i, j, *args, (0, 1, 5), c["frames_b"])       # pair 2 reads A's map 5 of 3
    bad_a = np.zeros(37, bool)
    bad_a[[3, 5]] = True
    bad_a[pair == 2] = True
    bad_b = np.zeros(37, bool)
    bad_b[[3, 7, 9]] = True
    for got, want, bad in ((wa, good[0], bad_a), (wb, good[1], bad_b)):
        bad_t = torch.from_numpy(bad).to(cuda_device)
        assert not got[bad_t].any() and torch.equal(got[~bad_t], want[~bad_t])


def test_chain_from_transformer_to_lift_matches(cuda_device):
    """FeatureTransformer -> match_descriptors(border_rm=0) -> refine -> to_pixels -> lift_matches at a 9 x 9
    grid (a 72-pixel image, 36 x 36 fine maps): the rows are accepted, edge cells included."""
    from bundlesdf_amd import frames as F, matching as M, transformer as T
    from bundlesdf_amd.fine import FineRefiner
    dev, h = cuda_device, 9
    gen = torch.Generator().manual_seed(4)
    ft = T.FeatureTransformer(O.TO.make_weights(31, 256, ("self", "cross")), d_model=256, layer_names=("self", "cross"), device=dev)
    r = FineRefiner(O.make_weights(32), device=dev)
    tok = torch.randn((3, h * h, 256), generator=gen)
    fine = torch.randn((3, 128, 4 * h, 4 * h), generator=gen).to(dev)
    pairs = np.array([(0, 1), (1, 2), (0, 2)])
    ta = tok[pairs[:, 0]].to(dev)
    tb = (tok[pairs[:, 0]] + 0.05 * torch.randn((3, h * h, 256), generator=gen)).to(dev)    # B's cells planted from A's
    da, db = ft.forward(ta, tb)
    cm = M.match_descriptors(da, db, (h, h), (h, h), border_rm=0, thr=0.0)
    fm = r.refine(cm, fine, fine, da, db, frames_a=pairs[:, 0], frames_b=pairs[:, 1])
    n = int(cm.n_matches.sum())
    assert n > 0 and tuple(fm.expec.shape) == (n, 3) and torch.isfinite(fm.expec).all()
    assert float(fm.expec[:, :2].abs().max()) <= 1.0 and float(fm.expec[:, 2].min()) > 0
    edge = (fm.i % h == 0) | (fm.i % h == h - 1) | (fm.i // h == 0) | (fm.i // h == h - 1)
    assert bool(edge.any())
    uv_a, uv_b, pair_start, conf = fm.to_pixels(scale=8)
    ca, cb, cs, cc = cm.to_pixels(scale=8)
    assert torch.equal(uv_a, ca) and torch.equal(pair_start, cs) and torch.equal(conf, cc)
    assert float((uv_b - cb).abs().max()) <= 4.0 and bool((uv_b != cb).any())
    depth = torch.full((3, 8 * h, 8 * h), 0.5)
    K = np.array([[100.0, 0.0, 35.5], [0.0, 100.0, 35.5], [0.0, 0.0, 1.0]])
    lifted = F.lift_matches(F.depth_geometry(depth, K, device=dev), pairs, uv_a, uv_b, pair_start)
    assert tuple(lifted.pts_b.shape) == (n, 3) and lifted.valid.dtype == torch.bool
    inside = ((uv_b >= 0) & (uv_b <= 8 * h - 1)).all(1)
    assert not bool((lifted.valid & ~inside).any()) and bool(lifted.valid.any())     # a pixel refined off the image is not lifted


def test_forward_inplace_equals_forward(cuda_device):
    from bundlesdf_amd import transformer as T
    c = O.TO.CASES["fine2"]
    w, a, b, _, _ = O.TO.case_data("fine2")
    ft = T.FeatureTransformer(w, d_model=c["C"], layer_names=c["layers"], device=cuda_device)
    ta, tb = torch.from_numpy(a).to(cuda_device), torch.from_numpy(b).to(cuda_device)
    want = ft.forward(ta, tb)
    xa, xb = ta.clone(), tb.clone()
    got = ft.forward_inplace(xa, xb)
    assert got[0] is xa and got[1] is xb and xa.data_ptr() == got[0].data_ptr()
    assert torch.equal(xa, want[0]) and torch.equal(xb, want[1])
    assert not torch.equal(xa, ta)                                          # the inputs were overwritten
