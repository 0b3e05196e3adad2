"""GPU: bundlesdf_amd.transformer (csrc/feature_transformer.hip, include/nof.h group 12) against the
reference's LocalFeatureTransformer.

The yardstick is tests/golden/feature_transformer*.npz: the reference module's float64 outputs on the
cases of tests/transformer_oracle.py, and its own half-precision error e16 (its output under fp16
autocast minus its float64 output, without masks). The kernels round to fp16 at other points than
autocast does, so the two errors are independent draws of the same size: the bound is 2 x e16, rms
and max, over all rows, masked ones included. A wrong head split, mask, scaling, LayerNorm or layer
order is off by order 1, several hundred times the bound."""
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
        rms, mx = _errors(out, golden[f"{case}_a{key}"], golden[f"{case}_b{key}"])
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
