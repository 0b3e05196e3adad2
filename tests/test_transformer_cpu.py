"""CPU: the feature transformer's oracle, fixture, position encoding, weight packing and argument checks.

tests/golden/feature_transformer*.npz holds what the reference's LocalFeatureTransformer gives in
float64 on the cases of tests/transformer_oracle.py (recorded by tests/golden/make_feature_transformer.py).
The oracle is the definition in csrc/feature_transformer.hip's header restated in float64: it must
reproduce the module to rounding, and it must see the cross-order bug the cross1 case exists for."""
import ctypes

import numpy as np
import pytest
import torch

from tests import transformer_oracle as O


@pytest.fixture(scope="module")
def golden(golden_dir):
    return O.load_golden(golden_dir)


@pytest.mark.parametrize("case", O.STORED)
def test_oracle_reproduces_the_reference_module(golden, case):
    """Two float64 evaluations of one formula: the error is O(1e-13), the bound 1e-9 absolute."""
    w, a, b, ma, mb = O.case_data(case)
    oa, ob = O.forward(w, O.CASES[case]["layers"], a, b)
    assert np.abs(oa - golden[f"{case}_a64"]).max() <= 1e-9
    assert np.abs(ob - golden[f"{case}_b64"]).max() <= 1e-9
    if ma is not None:
        oa, ob = O.forward(w, O.CASES[case]["layers"], a, b, ma, mb)
        assert np.isfinite(golden[f"{case}_a64m"]).all() and np.isfinite(golden[f"{case}_b64m"]).all()
        assert np.abs(oa - golden[f"{case}_a64m"]).max() <= 1e-9
        assert np.abs(ob - golden[f"{case}_b64m"]).max() <= 1e-9


def test_fixture_sees_the_cross_order(golden):
    """The two applications of a cross layer in the other order miss cross1 by far more than any
    half-precision error: the fixture can tell the two apart."""
    w, a, b, _, _ = O.case_data("cross1")
    oa, ob = O.forward(w, O.CASES["cross1"]["layers"], a, b, cross_b_first=True)
    err = max(np.abs(oa - golden["cross1_a64"]).max(), np.abs(ob - golden["cross1_b64"]).max())
    assert err > 100 * float(golden["cross1_e16_max"])


@pytest.mark.parametrize("case", list(O.CASES))
def test_fixture_holds_a_half_precision_error_for_every_case(golden, case):
    """e16 is what every GPU bound is a multiple of. It is a handful of fp16 roundings (each up to 2^-11
    relative) of values of the outputs' size: between 2^-13 and 2^-9 of the oracle's output rms, and its
    largest element within 16 rms. For the cases without stored outputs this ties the recorded scalars to
    the oracle's outputs of the same case."""
    e_rms, e_max = float(golden[f"{case}_e16_rms"]), float(golden[f"{case}_e16_max"])
    out = O.flat(O.case_output(case))
    rms = float(np.sqrt(np.mean(out ** 2)))
    assert np.isfinite(out).all() and 2.0 ** -13 * rms <= e_rms <= 2.0 ** -9 * rms, (case, e_rms, rms)
    assert e_rms <= e_max <= 16 * e_rms, (case, e_rms, e_max)


@pytest.mark.parametrize("mutant", list(O.MUTANTS))
def test_named_cases_tell_a_mutant_from_the_definition(golden, mutant):
    """rms(d_m) >= factor x e16_rms on every case the table names for the mutant: 6 for the structural ones
    (2 x e16 for the kernels plus the same again, with room), 1 for a wrong constant or divisor."""
    cases, factor = O.MUTANTS[mutant]
    for case in cases:
        d = O.mutant_delta(case, mutant)
        dist = float(np.sqrt(np.mean(d ** 2))) / float(golden[f"{case}_e16_rms"])
        print(f"{mutant} {case}: {dist:.1f} e16_rms")
        assert dist >= factor, (mutant, case, dist)


def test_eps_shows_only_in_the_amplifying_cases(golden):
    """At the ordinary weights a LayerNorm eps of 1e-6 is below e16: no bound on the output can see it. With
    merge.weight and mlp.2.weight scaled down, the variance both LayerNorms see is of the order of eps and the
    same mutant is hundreds of e16 away."""
    for mutant in ("ln1_eps", "ln2_eps"):
        d = O.mutant_delta("self1", mutant)
        assert np.sqrt(np.mean(d ** 2)) < float(golden["self1_e16_rms"])
        for case in ("amp256", "amp128"):
            d = O.mutant_delta(case, mutant)
            assert np.sqrt(np.mean(d ** 2)) > 100 * float(golden[f"{case}_e16_rms"])


def test_a_masked_query_is_x_plus_the_feed_forward_of_bias1():
    """The oracle's rows with mask 0: msg is exactly 0, LayerNorm1 of zeros is its bias, so the row is
    x + LN2(relu([x | bias1] W1^T) W2^T) and no source enters it."""
    case = "edge_64_65"
    w, a, b, ma, mb = O.case_data(case)
    g = lambda name: w["layers.0." + name].astype(np.float64)
    out_a = O.case_output(case, True)[0]
    assert (~ma).sum() > 0
    x = a.astype(np.float64)[~ma]
    hid = np.maximum(np.concatenate([x, np.broadcast_to(g("norm1.bias"), x.shape)], 1) @ g("mlp.0.weight").T, 0.0)
    y = hid @ g("mlp.2.weight").T
    mu = y.mean(-1, keepdims=True)
    ln2 = (y - mu) / np.sqrt(((y - mu) ** 2).mean(-1, keepdims=True) + 1e-5) * g("norm2.weight") + g("norm2.bias")
    assert np.abs(out_a[~ma] - (x + ln2)).max() <= 1e-12


@pytest.mark.parametrize("fix", [False, True])
def test_position_encoding_matches_the_reference(golden, fix):
    from bundlesdf_amd import transformer as T
    for C, h, w in O.PE_GRIDS:
        want = golden[f"pe_{C}_{h}x{w}_{int(fix)}"]                     # [C,h,w]
        got = T.position_encoding(h, w, C, temp_bug_fix=fix)
        assert got.shape == (h * w, C) and got.dtype == torch.float32
        assert np.abs(got.numpy() - want.transpose(1, 2, 0).reshape(h * w, C)).max() <= 1e-6


def test_add_position_encoding_is_feat_plus_pe_rearranged():
    import bundlesdf_amd
    T = bundlesdf_amd.transformer                                       # exported as matching is
    rng = np.random.default_rng(7)
    feat = rng.standard_normal((3, 128, 5, 9)).astype(np.float32)
    for fix in (False, True):
        pe = T.position_encoding(5, 9, 128, temp_bug_fix=fix).numpy()   # [hw,C]
        want = feat.transpose(0, 2, 3, 1).reshape(3, 45, 128) + pe[None]
        got = T.add_position_encoding(feat, temp_bug_fix=fix)
        assert got.shape == (3, 45, 128) and got.dtype == torch.float32
        np.testing.assert_array_equal(got.numpy(), want)
        np.testing.assert_array_equal(T.add_position_encoding(torch.from_numpy(feat).half(), fix).numpy(),
                                      feat.astype(np.float16).astype(np.float32).transpose(0, 2, 3, 1).reshape(3, 45, 128)
                                      + pe[None])
    assert not np.array_equal(T.position_encoding(5, 9, 128, True).numpy(), T.position_encoding(5, 9, 128, False).numpy())


def test_from_state_dict_prefixes_packing_and_rejections():
    from bundlesdf_amd import transformer as T
    names = ("self", "cross")
    w = O.make_weights(3, 128, names)
    plain = T.FeatureTransformer(w, d_model=128, layer_names=names)
    assert plain.packed.dtype == np.uint8 and plain.packed.size == 2 * T.layer_bytes(128)
    for prefix in ("loftr_coarse.", "loftr_fine.", "matcher.loftr_coarse."):
        sd = {prefix + k: torch.from_numpy(v) for k, v in w.items()}
        sd["backbone.conv1.weight"] = torch.zeros(4, 4)
        for given in (None, prefix):
            ft = T.FeatureTransformer.from_state_dict(sd, prefix=given, d_model=128, layer_names=names)
            np.testing.assert_array_equal(ft.packed, plain.packed)
    # a checkpoint with both transformers: the prefix is found by d_model
    both = {"loftr_fine." + k: v for k, v in w.items()}
    both.update({"loftr_coarse." + k: v for k, v in O.make_weights(4, 256, names).items()})
    np.testing.assert_array_equal(T.FeatureTransformer.from_state_dict(both, d_model=128, layer_names=names).packed,
                                  plain.packed)

    # the packed block: fragment order of the matrices, then the LayerNorm parameters in float32
    C = 128
    wq = plain.packed[:C * C * 2].view(np.float16).reshape(C // 32, C // 16, 64, 8)
    src = w["layers.0.q_proj.weight"]
    for nt, ks, lane, j in ((0, 0, 0, 0), (3, 7, 63, 7), (1, 2, 37, 5), (2, 5, 31, 1)):
        assert wq[nt, ks, lane, j] == src[32 * nt + lane % 32, 16 * ks + 8 * (lane // 32) + j]
    w1 = plain.packed[8 * C * C:16 * C * C].view(np.float16).reshape(2 * C // 32, 2 * C // 16, 64, 8)
    assert w1[5, 9, 40, 3] == w["layers.0.mlp.0.weight"][32 * 5 + 8, 16 * 9 + 8 + 3]
    ln = plain.packed[20 * C * C:T.layer_bytes(C)].view(np.float32).reshape(4, C)
    for row, key in enumerate(("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")):
        np.testing.assert_array_equal(ln[row], w["layers.0." + key])

    missing = dict(w)
    del missing["layers.1.merge.weight"]
    with pytest.raises(ValueError, match=r"layers\.1\.merge\.weight"):
        T.FeatureTransformer.from_state_dict(missing, d_model=128, layer_names=names)
    bad = dict(w)
    bad["layers.0.mlp.2.weight"] = np.zeros((128, 128), np.float32)
    with pytest.raises(ValueError, match=r"layers\.0\.mlp\.2\.weight"):
        T.FeatureTransformer.from_state_dict(bad, d_model=128, layer_names=names)
    with pytest.raises(ValueError, match="192"):
        T.FeatureTransformer.from_state_dict(w, d_model=192, layer_names=names)
    with pytest.raises(ValueError, match="full"):
        T.FeatureTransformer.from_state_dict(w, d_model=128, layer_names=("self", "full"))


def test_entry_point_refuses_bad_shapes_before_device_work():
    """NOF_EINVAL with the field named, on a machine with no GPU: the descriptor is validated before the
    first HIP call."""
    from bundlesdf_amd import _lib, build
    build.build()
    lib = _lib.lib()

    def desc(**kw):
        D = _lib.FeatureTransformerDesc()
        D.P, D.L, D.S, D.C, D.n_layers = 2, 70, 45, 256, 2
        D.layer_kind[0], D.layer_kind[1] = _lib.FT_SELF, _lib.FT_CROSS
        for k, v in kw.items():
            setattr(D, k, v)
        return D

    for kw, text in ((dict(C=192), b"C=192"), (dict(L=0), b"L=0"), (dict(n_layers=17), b"n_layers=17"),
                     (dict(S=0), b"S=0"), (dict(P=32768), b"P=32768"), (dict(), b"feat_a is NULL")):
        assert lib.nof_feature_transformer(ctypes.byref(desc(**kw)), None) != 0
        assert text in lib.nof_last_error(), (kw, lib.nof_last_error())
    D = desc()
    D.layer_kind[1] = 2
    assert lib.nof_feature_transformer(ctypes.byref(D), None) != 0
    assert b"layer_kind[1]=2" in lib.nof_last_error()
    assert lib.nof_feature_transformer_workspace_bytes(2, 70, 45, 192) == 0
    assert lib.nof_feature_transformer_workspace_bytes(2, 70, 45, 256) > 0
