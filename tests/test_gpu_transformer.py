"""GPU: bundlesdf_amd.transformer (csrc/feature_transformer.hip, include/nof.h group 12) against the
reference's LocalFeatureTransformer.

The yardstick is tests/golden/feature_transformer*.npz: the reference module's float64 outputs on the
cases of tests/transformer_oracle.py, and its own half-precision error e16 (its output under fp16
autocast minus its float64 output, without masks). The kernels round to fp16 at other points than
autocast does, so the two errors are independent draws of the same size: the bound is 2 x e16, rms
and max, over all rows, masked ones included. A wrong head split, mask, scaling, LayerNorm or layer
order is off by order 1, several hundred times the bound. The cases with stored=False (edge shapes, the
amplifying cases) are held to the same bound against the float64 oracle, which test_transformer_cpu.py ties
to the reference.

What that bound cannot see is held in two other ways. Exact claims (a row of x depends on no other row, a
masked source row carries nothing, a masked query gets the message 0) are torch.equal between two runs. Small
deviations (a LayerNorm constant or divisor: transformer_oracle.MUTANTS) are held by projection: the
component of the kernels' error along a mutant's deviation d_m is 1 for a kernel that is the mutant and
rounding noise over sqrt(n) for a correct one; the cap is 0.25, where the reference's own fp16 path stays
within 0.1 (asserted when the fixture is recorded)."""
import numpy as np
import pytest
import torch

from tests import transformer_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return O.load_golden(golden_dir)


_RUNS = {}


def _run(case, dev):
    """(FeatureTransformer, inputs, outputs without masks, outputs with masks or None), once per case."""
    from bundlesdf_amd import transformer as T
    if case not in _RUNS:
        c = O.CASES[case]
        w, a, b, ma, mb = O.case_data(case)
        ft = T.FeatureTransformer.from_state_dict(w, d_model=c["C"], layer_names=c["layers"], device=dev)
        ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        plain = ft.forward(ta, tb)
        masked = None if ma is None else ft.forward(ta, tb, ma, mb)
        torch.cuda.synchronize()
        _RUNS[case] = (ft, (ta, tb, ma, mb), plain, masked)
    return _RUNS[case]


def _want(golden, case, masked):
    """The float64 outputs a case is held to: the fixture's, or the oracle's where none are stored."""
    if O.CASES[case].get("stored", True):
        key = "64m" if masked else "64"
        return golden[f"{case}_a{key}"], golden[f"{case}_b{key}"]
    return O.case_output(case, masked)


def _errors(out, want_a, want_b):
    err = np.concatenate([(out[0].double().cpu().numpy() - want_a).ravel(), (out[1].double().cpu().numpy() - want_b).ravel()])
    return float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())


@pytest.mark.parametrize("case", list(O.CASES))
def test_against_the_reference_module(cuda_device, golden, case):
    _, _, plain, masked = _run(case, cuda_device)
    e_rms, e_max = float(golden[f"{case}_e16_rms"]), float(golden[f"{case}_e16_max"])
    runs = [("plain", plain, "64")] + ([("masked", masked, "64m")] if masked is not None else [])
    for label, out, key in runs:
        assert out[0].dtype == torch.float32 and out[1].dtype == torch.float32
        assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all()
        rms, mx = _errors(out, *_want(golden, case, key == "64m"))
        print(f"{case} {label}: rms {rms:.3e} = {rms / e_rms:.2f} e16_rms, max {mx:.3e} = {mx / e_max:.2f} e16_max")
        assert rms <= 2 * e_rms, (case, label, rms, e_rms)
        assert mx <= 2 * e_max, (case, label, mx, e_max)


@pytest.mark.parametrize("case", list(O.CASES))
def test_same_bytes_on_every_call_and_for_every_batching(cuda_device, case):
    ft, (ta, tb, ma, mb), plain, masked = _run(case, cuda_device)
    want = masked if masked is not None else plain
    again = ft.forward(ta, tb, ma, mb)
    assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1])
    for p in range(ta.shape[0]):            # the P pairs in P calls
        one = ft.forward(ta[p:p + 1], tb[p:p + 1], None if ma is None else ma[p:p + 1], None if mb is None else mb[p:p + 1])
        assert torch.equal(one[0][0], want[0][p]) and torch.equal(one[1][0], want[1][p]), p


@pytest.mark.parametrize("case", sorted({c for cases, _ in O.MUTANTS.values() for c in cases}))
def test_error_has_no_component_along_a_mutant(cuda_device, golden, case):
    """alpha_m = <out - oracle, d_m> / <d_m, d_m> for every mutant that names the case: a kernel that is the
    mutant gives 1, one that is half of it 0.5, zero-mean rounding noise (noise_rms / rms(d_m)) / sqrt(n)."""
    _, _, plain, masked = _run(case, cuda_device)
    use_masks = masked is not None
    out = masked if use_masks else plain
    err = O.flat([o.double().cpu().numpy() for o in out]) - O.flat(_want(golden, case, use_masks))
    for mutant, (cases, _) in O.MUTANTS.items():
        if case in cases:
            alpha = O.projection(err, O.mutant_delta(case, mutant))
            print(f"{case} {mutant}: alpha {alpha:+.4f}")
            assert abs(alpha) <= 0.25, (case, mutant, alpha)


# --- exact claims: one cross layer, the a output, torch.equal ---

def _cross_layer(C, dev):
    from bundlesdf_amd import transformer as T
    return T.FeatureTransformer.from_state_dict(O.make_weights(200 + C, C, ("cross",)), d_model=C, layer_names=("cross",),
                                                device=dev)


def _normal(rng, shape, dev, scale=1.0):
    return torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float16).astype(np.float32)).to(dev)


@pytest.mark.parametrize("C", [128, 256])
def test_a_row_of_x_depends_on_no_other_row(cuda_device, C):
    """L = 130 is tiles of 64, 64 and 2 rows. A subset or reordering of a's rows moves rows across tile edges,
    into and out of the tail tile and between lanes and registers; each must come out with the same bytes."""
    ft, rng, L, S = _cross_layer(C, cuda_device), np.random.default_rng(300 + C), 130, 70
    a, b = _normal(rng, (2, L, C), cuda_device), _normal(rng, (2, S, C), cuda_device)
    ma = torch.from_numpy(rng.random((2, L)) < 0.8).to(cuda_device)
    mb = torch.from_numpy(rng.random((2, S)) < 0.8).to(cuda_device)
    whole = ft.forward(a, b, ma, mb)[0]
    assert torch.isfinite(whole).all()
    lists = {"reversed": list(range(L - 1, -1, -1)), "63,64": [63, 64], "129": [129], "first 65": list(range(65)),
             "permuted": [int(i) for i in np.random.default_rng(7).permutation(L)]}
    for name, idx in lists.items():
        part = ft.forward(a[:, idx].contiguous(), b, ma[:, idx].contiguous(), mb)[0]
        assert torch.equal(part, whole[:, idx]), name


def _masks_b(pattern, rng):
    """pattern -> (S, mask_b [2,S] bool)."""
    if pattern == "tile_end":                       # the last 6 rows of the first 64-row tile
        S, dead = 70, slice(58, 64)
    elif pattern == "middle_tile":
        S, dead = 200, slice(64, 128)
    elif pattern == "second_block":                 # rows 256..511: one k_ft_kv block whose partial is all zeros
        S, dead = 520, slice(256, 512)
    else:
        return 70, rng.random((2, 70)) < 0.7
    m = np.ones((2, S), bool)
    m[:, dead] = False
    return S, m


@pytest.mark.parametrize("pattern", ["tile_end", "middle_tile", "second_block", "random"])
@pytest.mark.parametrize("C", [128, 256])
def test_a_masked_source_row_carries_nothing(cuda_device, C, pattern):
    """The masked rows of b hold 8 N(0,1) in one run and zeros in the other (moderate, so that elu stays
    finite: 0 x inf is NaN in the definition too): a comes out with the same bytes."""
    ft, rng, L = _cross_layer(C, cuda_device), np.random.default_rng(400 + C), 130
    S, mb_host = _masks_b(pattern, rng)
    a, b = _normal(rng, (2, L, C), cuda_device), _normal(rng, (2, S, C), cuda_device)
    ma = torch.from_numpy(rng.random((2, L)) < 0.8).to(cuda_device)
    mb = torch.from_numpy(mb_host).to(cuda_device)
    noisy = torch.where(mb[:, :, None], b, _normal(rng, (2, S, C), cuda_device, 8.0))
    zeroed = torch.where(mb[:, :, None], b, torch.zeros_like(b))
    assert not torch.equal(noisy, zeroed)
    out_noisy, out_zeroed = ft.forward(a, noisy, ma, mb)[0], ft.forward(a, zeroed, ma, mb)[0]
    assert torch.isfinite(out_noisy).all()
    assert torch.equal(out_noisy, out_zeroed)


@pytest.mark.parametrize("C", [128, 256])
def test_a_masked_row_of_a_self_layer_carries_nothing(cuda_device, C):
    """L = 300, S = 45: the sides have two and one KV blocks. What a masked row holds shows in that row's own
    output alone: the live rows of its side and the whole other side keep their bytes."""
    from bundlesdf_amd import transformer as T
    ft = T.FeatureTransformer.from_state_dict(O.make_weights(500 + C, C, ("self",)), d_model=C, layer_names=("self",),
                                              device=cuda_device)
    rng, L, S = np.random.default_rng(600 + C), 300, 45
    a, b = _normal(rng, (2, L, C), cuda_device), _normal(rng, (2, S, C), cuda_device)
    ma = torch.from_numpy(rng.random((2, L)) < 0.8).to(cuda_device)
    mb = torch.from_numpy(rng.random((2, S)) < 0.8).to(cuda_device)
    a0, b0 = torch.where(ma[:, :, None], a, torch.zeros_like(a)), torch.where(mb[:, :, None], b, torch.zeros_like(b))
    a8 = torch.where(ma[:, :, None], a, _normal(rng, (2, L, C), cuda_device, 8.0))
    b8 = torch.where(mb[:, :, None], b, _normal(rng, (2, S, C), cuda_device, 8.0))
    base = ft.forward(a0, b0, ma, mb)
    on_a, on_b = ft.forward(a8, b0, ma, mb), ft.forward(a0, b8, ma, mb)
    assert all(torch.isfinite(o).all() for o in base + on_a + on_b)
    assert torch.equal(on_a[0][ma], base[0][ma]) and torch.equal(on_a[1], base[1])
    assert torch.equal(on_b[1][mb], base[1][mb]) and torch.equal(on_b[0], base[0])
    assert not torch.equal(on_a[0], base[0]) and not torch.equal(on_b[1], base[1])


@pytest.mark.parametrize("case", ["edge_64_65", "fine_128_257"])
def test_a_masked_query_gets_the_message_zero(cuda_device, golden, case):
    """A row of a with mask 0 has msg exactly 0, so LayerNorm1 gives its bias and the row is
    x + LN2(relu([x | bias1] W1^T) W2^T), whatever the source: finite, the same bytes for another source of
    another length, and within the case's bound of the oracle's rows."""
    ft, (ta, tb, ma, mb), _, masked = _run(case, cuda_device)
    dead = torch.from_numpy(~ma).to(cuda_device)
    assert int(dead.sum()) > 0
    rows = masked[0][dead]
    assert torch.isfinite(rows).all()
    rng = np.random.default_rng(9)
    other = ft.forward(ta, _normal(rng, (ta.shape[0], 33, ta.shape[2]), cuda_device), ma, None)[0]
    assert torch.equal(other[dead], rows)
    err = rows.double().cpu().numpy() - _want(golden, case, True)[0][~ma]
    rms, mx = float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())
    e_rms, e_max = float(golden[f"{case}_e16_rms"]), float(golden[f"{case}_e16_max"])
    print(f"{case} masked queries: rms {rms / e_rms:.2f} e16_rms, max {mx / e_max:.2f} e16_max")
    assert rms <= 2 * e_rms and mx <= 2 * e_max, (case, rms, mx)


@pytest.mark.parametrize("case", ["self1", "fine2"])
def test_float16_input_equals_float32_input(cuda_device, case):
    ft, (ta, tb, _, _), plain, _ = _run(case, cuda_device)
    half = ft.forward(ta.half(), tb.half())                 # the inputs hold fp16 values
    assert torch.equal(half[0], plain[0]) and torch.equal(half[1], plain[1])
    host = ft.forward(ta.cpu().numpy(), tb.cpu().numpy())   # numpy in, device tensors out
    assert host[0].is_cuda and torch.equal(host[0], plain[0]) and torch.equal(host[1], plain[1])
    single = ft.forward(ta[0], tb[0])                       # one pair without the P axis
    assert single[0].shape == (1,) + tuple(ta.shape[1:]) and torch.equal(single[0][0], plain[0][0])


def test_outputs_go_into_match_descriptors(cuda_device):
    from bundlesdf_amd import matching as M
    _, _, plain, _ = _run("coarse8", cuda_device)
    m = M.match_descriptors(plain[0], plain[1], (7, 10), (5, 9))
    assert tuple(m.j_of_i.shape) == (2, 70) and m.j_of_i.dtype == torch.int32
    assert int(m.n_matches.min()) >= 0 and int(m.j_of_i.max()) < 45


def test_workspace_is_cached_and_grown(cuda_device):
    ft, (ta, tb, _, _), plain, _ = _run("cross1", cuda_device)
    ws = ft._workspace[plain[0].device]
    ft.forward(ta[:1, :8], tb[:1, :8])
    assert ft._workspace[plain[0].device] is ws
