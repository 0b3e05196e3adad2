"""CPU: the backbone's oracle, fixture, weight folding and packing, key lookup, argument checks, scratch layout
and LoftrRunner's host side.

tests/golden/backbone*.npz holds what the reference's ResNetFPN_8_2 gives in float64 on the cases of
tests/backbone_oracle.py (recorded by tests/golden/make_backbone.py). The oracle is the definition in
csrc/backbone.hip's header restated in float64: it must reproduce the module to rounding."""
import ctypes

import numpy as np
import pytest
import torch

from tests import backbone_oracle as O

EINVAL = 1
DUMMY = 0x1000      # a non-null, 16-byte aligned address that is never read: every call below is refused first


@pytest.fixture(scope="module")
def golden(golden_dir):
    return O.load_golden(golden_dir)


@pytest.fixture(scope="module")
def weights():
    return O.make_weights()


@pytest.mark.parametrize("case", list(O.CASES))
def test_oracle_reproduces_the_reference_module(golden, weights, case):
    """Two float64 evaluations of one network: the error is O(1e-14) of the output's rms, the bound 1e-9."""
    c = O.CASES[case]
    images = O.make_images(case)
    np.testing.assert_array_equal(images, golden[f"{case}_images"])
    coarse, fine = O.forward(weights, images)
    assert coarse.shape == (c["N"], 256, c["H"] // 8, c["W"] // 8) and fine.shape == (c["N"], 128, c["H"] // 2, c["W"] // 2)
    for key, got in (("coarse", coarse), ("fine", fine)):
        want = golden[f"{case}_{key}64"]
        rms = np.sqrt(np.mean(want ** 2))
        assert rms >= 0.1 and float(golden[f"{case}_{key}_e16_max"]) < rms / 20
        assert np.abs(got - want).max() <= 1e-9 * rms, (case, key)


def test_rounding_model_stays_within_the_device_bound(golden, weights):
    """The oracle with the device's rounding points misses the fixture by less than the 2 x e16 the device is
    held to, at the smallest case: the bound is reachable by the arithmetic the header states."""
    coarse, fine = O.forward(weights, O.make_images("one_cell"), rounded=True)
    for key, got in (("coarse", coarse), ("fine", fine)):
        err = got - golden[f"one_cell_{key}64"]
        assert np.sqrt(np.mean(err ** 2)) <= 2 * float(golden[f"one_cell_{key}_e16_rms"])
        assert np.abs(err).max() <= 2 * float(golden[f"one_cell_{key}_e16_max"])


def test_fold_batchnorm_and_pack_conv(weights):
    from bundlesdf_amd import backbone as B
    w = weights
    # the fold against BatchNorm applied after the convolution, on one pixel's patch
    rng = np.random.default_rng(5)
    p = "layer2.0."
    W = w[p + "conv1.weight"]
    bn = [w[p + "bn1." + k] for k in ("weight", "bias", "running_mean", "running_var")]
    Wf, b = B.fold_batchnorm(W, *bn)
    assert Wf.dtype == np.float16 and b.dtype == np.float32 and Wf.shape == W.shape and b.shape == (196,)
    x = rng.standard_normal(W.shape[1:])
    y = (W.astype(np.float64) * x).sum((1, 2, 3))
    want = (y - bn[2]) / np.sqrt(bn[3].astype(np.float64) + 1e-5) * bn[0] + bn[1]
    got = (Wf.astype(np.float64) * x).sum((1, 2, 3)) + b
    exact = W.astype(np.float64) * (bn[0].astype(np.float64) / np.sqrt(bn[3].astype(np.float64) + 1e-5))[:, None, None, None]
    # every weight within half an fp16 ulp (2^-11 relative) of the float64 fold, b' within half a float32 ulp
    assert (np.abs(got - want) <= 2.0 ** -11 * np.abs(exact * x).sum((1, 2, 3)) + 2.0 ** -24 * np.abs(want) + 1e-7).all()
    np.testing.assert_array_equal(Wf, exact.astype(np.float16))                       # rounded once, from float64

    # the matrix: k = (ky KW + kx) Cin_p + c, pad rows and columns zero, the skip's columns after the taps
    skip = w[p + "downsample.0.weight"].astype(np.float16)
    W2 = w[p + "conv2.weight"].astype(np.float16)
    M = B.conv_matrix(W2, skip)
    assert M.shape == (224, 9 * 224 + 128) and M.dtype == np.float16
    for o, c, ky, kx in ((0, 0, 0, 0), (195, 195, 2, 2), (17, 100, 1, 2), (64, 31, 2, 0)):
        assert M[o, (ky * 3 + kx) * 224 + c] == W2[o, c, ky, kx]
    np.testing.assert_array_equal(M[:196, 9 * 224:], skip[:, :, 0, 0])
    assert not M[196:].any() and not M[:, :9 * 224].reshape(224, 9, 224)[:, :, 196:].any()
    stem = B.conv_matrix(w["conv1.weight"].astype(np.float16))
    assert stem.shape == (128, 64) and not stem[:, 49:].any()
    np.testing.assert_array_equal(stem[:, :49].reshape(128, 7, 7), w["conv1.weight"][:, 0].astype(np.float16))

    # the fragment order of csrc/mfma_tile.h, entry by entry, and back
    packed = B.pack_conv(W2, skip)
    NT, KS = 224 // 32, M.shape[1] // 16
    assert packed.shape == (NT, KS, 64, 8) and packed.dtype == np.float16
    nt, ks, lane, j = np.meshgrid(np.arange(NT), np.arange(KS), np.arange(64), np.arange(8), indexing="ij")
    np.testing.assert_array_equal(packed, M[32 * nt + lane % 32, 16 * ks + 8 * (lane // 32) + j])
    unpacked = np.zeros_like(M)
    unpacked[32 * nt + lane % 32, 16 * ks + 8 * (lane // 32) + j] = packed
    np.testing.assert_array_equal(unpacked, M)


def test_packed_buffer_follows_the_layout(weights):
    from bundlesdf_amd import _lib, backbone as B, build
    build.build()
    bb = B.Backbone(weights)
    layout, total = B.weight_layout()
    assert bb.packed.dtype == np.uint8 and bb.packed.size == total == _lib.lib().nof_backbone_weights_bytes()
    assert len(layout) == len(B.LAYERS) == 20 and all(w % 128 == 0 and b % 128 == 0 for w, b, _, _ in layout)
    # layer 6: layer2.0.conv2 with the block's shortcut and the sum of the two biases
    w_at, b_at, cout_p, K = layout[6]
    assert B.LAYERS[6] == ("layer2.0.conv2", "layer2.0.bn2", ("layer2.0.downsample.0", "layer2.0.downsample.1"))
    bn = lambda n: [weights[f"layer2.0.{n}.{k}"] for k in ("weight", "bias", "running_mean", "running_var")]
    W2, b2 = B.fold_batchnorm(weights["layer2.0.conv2.weight"], *bn("bn2"))
    Wd, bd = B.fold_batchnorm(weights["layer2.0.downsample.0.weight"], *bn("downsample.1"))
    assert (cout_p, K) == (224, 9 * 224 + 128)
    np.testing.assert_array_equal(bb.packed[w_at:b_at].view(np.float16), B.pack_conv(W2, Wd).ravel())
    bias = bb.packed[b_at:b_at + 4 * cout_p].view(np.float32)
    np.testing.assert_array_equal(bias[:196], b2 + bd)
    assert not bias[196:].any()
    # a convolution with no BatchNorm after it: rounded to fp16, bias zero
    w_at, b_at, cout_p, K = layout[19]
    np.testing.assert_array_equal(bb.packed[w_at:b_at].view(np.float16),
                                  B.pack_conv(weights["layer1_outconv2.3.weight"].astype(np.float16)).ravel())
    assert not bb.packed[b_at:b_at + 4 * cout_p].any() and b_at + 4 * cout_p == total


def test_from_state_dict_prefixes_and_rejections(weights):
    from bundlesdf_amd import backbone as B
    plain = B.Backbone(weights)
    for prefix in ("backbone.", "matcher.backbone.", ""):
        sd = {prefix + k: torch.from_numpy(v) for k, v in weights.items()}
        sd["loftr_coarse.layers.0.q_proj.weight"] = torch.zeros(4, 4)
        sd[prefix + "bn1.num_batches_tracked"] = torch.tensor(7)
        for given in (None, prefix):
            np.testing.assert_array_equal(B.Backbone.from_state_dict(sd, prefix=given).packed, plain.packed)
    for key in ("layer3.0.downsample.1.running_var", "conv1.weight", "layer1_outconv2.3.weight"):
        missing = dict(weights)
        del missing[key]
        with pytest.raises(ValueError, match=key.replace(".", r"\.") + ".*missing"):
            B.Backbone.from_state_dict(missing, prefix="")
    bad = dict(weights)
    bad["layer2_outconv.weight"] = np.zeros((256, 192, 1, 1), np.float32)
    with pytest.raises(ValueError, match=r"layer2_outconv\.weight.*\(256, 192, 1, 1\)"):
        B.Backbone(bad)
    with pytest.raises(ValueError, match="missing under every prefix"):
        B.Backbone.from_state_dict({"layers.0.q_proj.weight": np.zeros((4, 4))})


def _desc(**kw):
    from bundlesdf_amd import _lib
    L = _lib.lib()
    D = _lib.BackboneDesc()
    D.N, D.H, D.W = 2, 40, 56
    D.images = D.weights = D.pe = D.coarse = D.fine = D.scratch = DUMMY
    D.weights_bytes = L.nof_backbone_weights_bytes()
    D.scratch_bytes = L.nof_backbone_scratch_bytes(2, 40, 56)
    for k, v in kw.items():
        setattr(D, k, v)
    return D


def test_entry_point_refuses_bad_descriptors_before_device_work():
    """NOF_EINVAL with the field named, on a machine with no GPU: the descriptor is validated before the
    first HIP call."""
    from bundlesdf_amd import _lib, build
    build.build()
    L = _lib.lib()
    assert L.nof_backbone(None, None) == EINVAL and L.nof_last_error() == b"backbone: desc is NULL"
    cases = [(dict(N=0), b"N=0"), (dict(H=36), b"H=36"), (dict(W=4104), b"W=4104"), (dict(H=0), b"H=0")]
    cases += [({name: 0}, f"backbone: {name} is NULL".encode()) for name in ("images", "weights", "coarse", "fine", "scratch")]
    cases += [({name: DUMMY + 8}, f"backbone: {name} must be 16-byte aligned".encode())
              for name in ("images", "weights", "pe", "coarse", "fine", "scratch")]
    cases += [(dict(weights_bytes=L.nof_backbone_weights_bytes() - 1), b"weights_bytes="),
              (dict(scratch_bytes=L.nof_backbone_scratch_bytes(2, 40, 56) - 1), b"scratch_bytes=")]
    for kw, text in cases:
        assert L.nof_backbone(ctypes.byref(_desc(**kw)), None) == EINVAL, kw
        assert text in L.nof_last_error(), (kw, L.nof_last_error())


def test_scratch_bytes_equal_the_restated_layout():
    from bundlesdf_amd import _lib, backbone as B, build
    build.build()
    L = _lib.lib()
    shapes = [(c["N"], c["H"], c["W"]) for c in O.CASES.values()] + [(15, 480, 640), (64, 4096, 4096)]
    for N, H, W in shapes:
        assert L.nof_backbone_scratch_bytes(N, H, W) == B.scratch_bytes(N, H, W), (N, H, W)
    assert B.scratch_bytes(1, 8, 8) == 16 * (128 + 224 + 224) * 2 + 4 * (224 + 256 + 256) * 2 + 3 * 512
    assert B.scratch_bytes(64, 4096, 4096) > 1 << 32                # a product formed in 32 bits shows
    for N, H, W in ((0, 40, 56), (1, 36, 56), (1, 40, 4104), (1, 40, 60), (-1, 8, 8), (1, 0, 8)):
        assert L.nof_backbone_scratch_bytes(N, H, W) == 0, (N, H, W)
    assert not any(n.startswith("nof_backbone") and n.endswith("_workspace_bytes") for n in _lib.declared_symbols())


def test_forward_refuses_bad_shapes_on_the_host(weights):
    from bundlesdf_amd import backbone as B
    bb = B.Backbone(weights)
    for images, text in ((np.zeros((1, 36, 40), np.float32), "36x40"), (np.zeros((40, 40), np.float32), r"\(40, 40\)"),
                         (np.zeros((1, 3, 40, 40), np.float32), r"\(1, 3, 40, 40\)"),
                         (np.zeros((1, 40, 40), np.uint8), "floating-point"), (np.zeros((0, 40, 40), np.float32), "N=0")):
        with pytest.raises(ValueError, match=text):
            bb.forward(images)


# ---- the integer construction, the one-layer bound and the scratch views that tests/test_gpu_backbone.py uses ----

EXACT_LAYERS = {"trunk": tuple(range(14)), "head": tuple(range(13)) + (14, 15, 17, 18)}     # exact in that run
# what the GPU tests compare with the oracle in each run
COMPARED = {"trunk": ("layer1.1.conv2", "layer2.1.conv2", "layer3.1.conv2", "layer3.0.conv2", "layer3_outconv", "coarse"),
            "head": ("layer2_outconv2.0", "layer1_outconv", "layer1_outconv2.0")}
LRELU_LAYERS = ("layer2_outconv2.0", "layer1_outconv2.0")


@pytest.fixture(scope="module")
def exact_traces():
    """(kind, case) -> (weights, images, trace of the rounded oracle)."""
    out = {}
    for kind in ("trunk", "head"):
        w = O.exact_weights(kind)
        for case in ("ragged", "one_cell"):
            images, trace = O.exact_images(case), {}
            O.forward(w, images, rounded=True, trace=trace)
            out[kind, case] = (w, images, trace)
    return out


def test_exact_weights_fold_to_themselves_and_cover_every_column():
    from bundlesdf_amd import backbone as B
    w = O.exact_weights("trunk")
    for li in range(20):
        name, bn, skip, _, _ = O.layer_spec(li)
        for conv_name, bn_name in ((name, bn),) + ((skip,) if skip else ()):
            W = w[conv_name + ".weight"]
            assert np.isin(W, (-1.0, 0.0, 1.0)).all() and W.any()
            Wf, b = O.fold(w, conv_name, bn_name)
            np.testing.assert_array_equal(Wf, W)
            if bn_name is None:
                assert not b.any()
                continue
            bias = w[bn_name + ".bias"]
            np.testing.assert_array_equal(b, bias)
            assert (bias == np.round(bias)).all() and (np.diff(bias) != 0).all()        # a permuted bias shows
            Wd, bd = B.fold_batchnorm(W, *(w[f"{bn_name}.{k}"] for k in ("weight", "bias", "running_mean", "running_var")))
            np.testing.assert_array_equal(Wd.astype(np.float64), W)                      # the device's own fold too
            np.testing.assert_array_equal(bd, bias)
    for name, (cout, cin, k) in O.conv_shapes().items():
        W = w[name + ".weight"]
        if cin == 1:
            assert (W != 0).any(axis=(0, 1)).all() and k == 7                             # each of the 49 taps
        elif cout >= cin:
            assert (W != 0).any(axis=0).all(), name                                       # each (tap, channel) column
    head = O.exact_weights("head")
    zeroed = {"layer3_outconv.weight", "layer2_outconv2.3.weight"}
    for key in w:
        assert (not head[key].any()) if key in zeroed else np.array_equal(head[key], w[key]), key


@pytest.mark.parametrize("case", ["ragged", "one_cell"])
@pytest.mark.parametrize("kind", ["trunk", "head"])
def test_exact_runs_meet_their_conditions(exact_traces, kind, case):
    """What makes the integer runs exact, and what makes them worth running. Shares of non-zero entries that
    the numpy oracle gives: "ragged" 0.08 .. 0.15 in every relu layer; "one_cell" (a single pixel at 1/8,
    where a 3x3 sum is one tap) 0.031 in x1, x2, x3, layer3.0's output and coarse, which is the one channel
    in 32 with a positive bias, so there only "not entirely zero" is required."""
    w, images, trace = exact_traces[kind, case]
    assert (images == np.round(images)).all() and images.min() >= 0 and images.max() <= 7
    for li in EXACT_LAYERS[kind]:
        name = O.LAYER_NAMES[li]
        v = trace[name]
        whole = v == np.round(v)
        if name in LRELU_LAYERS:                             # the negative branch: fp16(0.01f * integer)
            assert whole[v >= 0].all() and (np.abs(v[v < 0]) < 2048 * 0.0101).all(), name
            np.testing.assert_array_equal(v, v.astype(np.float16).astype(np.float64))
        else:
            assert whole.all(), name
        assert np.abs(v).max() < 2048, (name, np.abs(v).max())
        ref, A = O.layer_reference(w, li, **O.layer_inputs(li, trace, images))
        assert A.max() < 2 ** 24, name                       # sum |w x| + |b'| + |res|: every partial sum is exact
        same = v >= 0 if name in LRELU_LAYERS else np.ones(v.shape, bool)   # float64 0.01f s may round otherwise
        np.testing.assert_array_equal(ref.astype(np.float16).astype(np.float64)[same], v[same], err_msg=name)
    if kind == "trunk":
        c = trace["coarse"]
        assert (c == np.round(c)).all() and np.abs(c).max() < 2 ** 24
    else:
        assert not trace["coarse"].any() and not trace["layer2_outconv2.3"].any() and not trace["layer3_outconv"].any()
    for name in COMPARED[kind]:
        share = float(np.mean(trace[name] != 0))
        print(f"{kind} {case} {name}: non-zero {share:.3f}, max {np.abs(trace[name]).max():.0f}")
        assert share >= (0.05 if case == "ragged" else 1e-9), (name, share)
    if case == "ragged":
        if kind == "trunk":
            assert len(np.unique(trace["coarse"])) >= 100
        else:
            s2 = trace["layer1_outconv2.0"]
            assert (s2 > 0).mean() > 0.05 and (s2 < 0).mean() > 0.05


def _emulate(w, li, x, skip=None, res=None, up=None, alter=None):
    """One layer as the kernel computes it, in numpy: a float32 accumulator that takes the taps in (ky, kx)
    order and the channels ascending within a tap, the fused skip after the last tap, then the float32
    epilogue and one rounding to fp16 -> [N,ho,wo,Cout] fp16. Inputs are fp16, real channels only.
    alter: "res_after_round" rounds to fp16 before the residual is added; "skip_rounded" accumulates the
    skip on its own, rounds it to fp16 and adds it."""
    f32 = np.float32
    name, bn, sk, stride, act = O.layer_spec(li)

    def accumulate(acc, src, W, stride):
        cout, cin, k, _ = W.shape
        pad = k // 2
        N, H, Wd, _ = src.shape
        ho, wo = (H + 2 * pad - k) // stride + 1, (Wd + 2 * pad - k) // stride + 1
        sp = np.pad(src.astype(f32), ((0, 0), (pad, pad), (pad, pad), (0, 0)))
        Wf = W.astype(f32)
        for ky in range(k):
            for kx in range(k):
                tap = sp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride, :]
                for c in range(cin):
                    acc = acc + tap[..., c:c + 1] * Wf[:, c, ky, kx]          # the product is exact, the sum rounds
        return acc

    W, b = O.fold(w, name, bn)
    N, H, Wd, _ = x.shape
    acc = accumulate(np.zeros((N, H // stride, Wd // stride, W.shape[0]), f32), x, W, stride)
    if sk is not None:
        Wd_, bd = O.fold(w, *sk)
        b = (b.astype(f32) + bd.astype(f32))
        if alter == "skip_rounded":
            acc = acc + accumulate(np.zeros_like(acc), skip, Wd_, 2).astype(np.float16).astype(f32)
        else:
            acc = accumulate(acc, skip, Wd_, 2)
    v = acc + b.astype(f32)
    if res is not None:
        if alter == "res_after_round":
            v = v.astype(np.float16).astype(f32)
        v = v + res.astype(f32)
    if up is not None:
        v = v + O._up2(up, f32, f32)
    assert v.dtype == f32
    if act == "relu":
        v = np.maximum(v, f32(0))
    if act == "lrelu":
        v = np.where(v > 0, v, f32(O.LRELU) * v)
    return v.astype(np.float16)


def _ratio(w, li, got, **inputs):
    ref, A = O.layer_reference(w, li, **inputs)
    got = got.astype(np.float64)
    return np.abs(got - ref) / O.layer_bound(li, got, ref, A)


def _random_inputs(seed, **shapes):
    rng = np.random.default_rng(seed)
    return {k: np.maximum(rng.standard_normal(s), 0.0).astype(np.float16) if k != "up"
            else rng.standard_normal(s).astype(np.float16) for k, s in shapes.items()}


def test_stand_in_meets_the_one_layer_bound_and_slips_do_not(weights):
    """Without a GPU: the bound of test_one_layer_from_the_devices_own_input is reachable by float32
    accumulation in the kernel's order."""
    # layer 8, layer2.1.conv2: 3x3, 196 (224) -> 196 (224) on 8 x 8, with a residual
    a = _random_inputs(21, x=(1, 8, 8, 196), res=(1, 8, 8, 196))
    good = _ratio(weights, 8, _emulate(weights, 8, **a), **a)
    print(f"layer 8: max err / bound {good.max():.3f}")
    assert (good <= 1.0).all()
    # layer 17, layer1_outconv: 1x1, 128 -> 196 (224), EP_UP from a 4 x 4 map
    a = _random_inputs(22, x=(1, 8, 8, 128), up=(1, 4, 4, 196))
    good = _ratio(weights, 17, _emulate(weights, 17, **a), **a)
    print(f"layer 17: max err / bound {good.max():.3f}")
    assert (good <= 1.0).all()
    # layer 6, layer2.0.conv2 with the fused 1x1 stride-2 skip
    a = _random_inputs(23, x=(1, 8, 8, 196), skip=(1, 16, 16, 128))
    good = _ratio(weights, 6, _emulate(weights, 6, **a), **a)
    print(f"layer 6: max err / bound {good.max():.3f}")
    assert (good <= 1.0).all()


def test_residual_added_after_a_rounding_fails_the_exact_comparison():
    """At K = 2016 the float32 term of the one-layer bound is some ten fp16 half-ulps of a typical output, so a
    second rounding before the residual stays inside it (measured here: 0.38 of the bound). The exact
    comparison sees it: with ternary weights and integer inputs up to 2000 the sum before the residual
    passes 2048 and is odd half the time, float32 holds it exactly and fp16 does not."""
    w = O.exact_weights("trunk")
    rng = np.random.default_rng(24)
    a = {k: rng.integers(0, 2001, (1, 8, 8, 196)).astype(np.float16) for k in ("x", "res")}
    ref, A = O.layer_reference(w, 8, **a)
    assert A.max() < 2 ** 24 and (ref == np.round(ref)).all() and (ref > 2048).mean() > 0.05
    np.testing.assert_array_equal(_emulate(w, 8, **a), ref.astype(np.float16))
    assert (_emulate(w, 8, alter="res_after_round", **a) != ref.astype(np.float16)).any()


def test_skip_rounded_on_its_own_fails_the_exact_comparison():
    """The same for the fused 1x1 stride-2 skip of layer2.0.conv2 (0.31 of the one-layer bound when rounded on
    its own). The shortcut here sums eight channels, so that it is no fp16 value by itself."""
    w = dict(O.exact_weights("trunk"))
    Wd = w["layer2.0.downsample.0.weight"].copy()
    Wd[:, :8, 0, 0] = 1.0
    w["layer2.0.downsample.0.weight"] = Wd
    rng = np.random.default_rng(25)
    a = {"x": rng.integers(0, 2001, (1, 8, 8, 196)).astype(np.float16),
         "skip": rng.integers(0, 2001, (1, 16, 16, 128)).astype(np.float16)}
    ref, A = O.layer_reference(w, 6, **a)
    assert A.max() < 2 ** 24 and (ref == np.round(ref)).all() and (ref > 2048).mean() > 0.05
    np.testing.assert_array_equal(_emulate(w, 6, **a), ref.astype(np.float16))
    assert (_emulate(w, 6, alter="skip_rounded", **a) != ref.astype(np.float16)).any()


def test_stand_in_equals_the_oracle_bit_for_bit_under_integer_weights(exact_traces):
    w, images, trace = exact_traces["head", "ragged"]
    for li in (6, 8, 15, 17):                # the fused skip, a residual, lrelu, EP_UP with a zero up term
        inputs = {k: None if v is None else v[:1].astype(np.float16) for k, v in O.layer_inputs(li, trace, images).items()}
        got = _emulate(w, li, **inputs)
        np.testing.assert_array_equal(got.astype(np.float64), trace[O.LAYER_NAMES[li]][:1], err_msg=str(li))


def test_scratch_views_follow_the_layout():
    from bundlesdf_amd import backbone as B
    for N, H, W in [(c["N"], c["H"], c["W"]) for c in O.CASES.values()] + [(3, 16, 8)]:
        offsets, total = O.scratch_offsets(N, H, W)
        assert total == B.scratch_bytes(N, H, W) and list(offsets) == [p[0] for p in O.SCRATCH_PARTS]
        # a buffer put together part by part, each rounded up to 256 bytes, with a value that names its place
        p2 = N * (H // 2) * (W // 2)
        sized = [(p2, 128), (p2, 224), (p2, 224), (p2 // 4, 224), (p2 // 4, 256), (p2 // 4, 256)] + [(p2 // 16, 256)] * 3
        chunks, want, at = [], {}, 0
        for i, ((pix, c), (name, level, _, cp)) in enumerate(zip(sized, O.SCRATCH_PARTS)):
            assert offsets[name] == (at, (N, H // level, W // level, cp)) and at % 256 == 0
            part = np.full((pix * c * 2 + 255) // 256 * 256 // 2, -1.0, np.float16)
            want[name] = (i * 100 + np.arange(pix * cp) % 97).astype(np.float16)
            part[:pix * cp] = want[name]
            chunks.append(part)
            at += part.nbytes
        buf = np.concatenate(chunks + [np.zeros(64, np.float16)]).view(np.uint8)      # longer than the call needs
        for views in (O.scratch_views(buf, N, H, W), O.scratch_views(torch.from_numpy(buf), N, H, W)):
            for name, level, _, cp in O.SCRATCH_PARTS:
                v = np.asarray(views[name])
                assert v.shape == (N, H // level, W // level, cp) and v.dtype == np.float16
                np.testing.assert_array_equal(v.ravel(), want[name])
        views = O.scratch_views(buf, N, H, W)
        views["m1"][...] = 7                                                            # a view, not a copy
        assert (buf.view(np.float16)[offsets["m1"][0] // 2:][:views["m1"].size] == 7).all()
    with pytest.raises(AssertionError):
        O.scratch_views(np.zeros(B.scratch_bytes(1, 8, 8) - 1, np.uint8), 1, 8, 8)


class _FakeMatches:
    """What pack_corres reads of a FineMatches."""

    def __init__(self, uv_a, uv_b, pair_start, conf):
        self.parts = (torch.from_numpy(uv_a), torch.from_numpy(uv_b), torch.tensor(pair_start, dtype=torch.int32),
                      torch.from_numpy(conf))

    def to_pixels(self, rounded=True):
        assert rounded is False
        return self.parts


def test_loftr_runner_grey_conversion_and_packing(monkeypatch):
    """LoftrRunner with the device stages stubbed: what reaches Loftr.match and what comes back."""
    from bundlesdf_amd.compat import loftr_wrapper as LW
    rng = np.random.default_rng(11)
    rgb_a = rng.integers(0, 256, (3, 16, 24, 3)).astype(np.uint8)
    rgb_b = rng.integers(0, 256, (3, 16, 24, 3)).astype(np.uint8)
    grey = LW.to_grey(rgb_a)
    assert grey.dtype == np.float32 and grey.shape == (3, 16, 24)
    want = (0.2989 * rgb_a[..., 0].astype(np.float64) + 0.587 * rgb_a[..., 1] + 0.114 * rgb_a[..., 2]) / 255.0
    assert np.abs(grey - want).max() <= 4 * 2.0 ** -24
    np.testing.assert_array_equal(LW.to_grey(rgb_a.astype(np.float64)), grey)
    np.testing.assert_array_equal(LW.to_grey(rgb_a[..., :1]), rgb_a[..., 0].astype(np.float32) / np.float32(255.0))
    with pytest.raises(ValueError, match=r"\(3, 16, 24, 2\)"):
        LW.to_grey(rgb_a[..., :2])

    uv_a = rng.uniform(0, 24, (5, 2))
    uv_b = rng.uniform(0, 24, (5, 2))
    conf = rng.uniform(0, 1, 5).astype(np.float32)
    seen = {}

    class Stub:
        def match(self, images, pairs, thr):
            seen.update(images=images, pairs=pairs, thr=thr)
            return _FakeMatches(uv_a, uv_b, [0, 2, 2, 5], conf)

    monkeypatch.setattr(LW.Loftr, "from_state_dict", classmethod(lambda cls, sd, device=None: Stub()))
    runner = LW.LoftrRunner({"state_dict": {}})
    out = runner.predict(rgb_a, rgb_b)
    assert seen["thr"] == 0.2 and seen["pairs"].tolist() == [[0, 3], [1, 4], [2, 5]]
    np.testing.assert_array_equal(seen["images"], np.concatenate([grey, LW.to_grey(rgb_b)]))
    assert [o.shape for o in out] == [(2, 5), (0, 5), (3, 5)] and all(o.dtype == np.float32 for o in out)
    rows = np.concatenate([uv_a, uv_b, conf[:, None].astype(np.float64)], 1).astype(np.float32)
    np.testing.assert_array_equal(np.concatenate(out), rows)
