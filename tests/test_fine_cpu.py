"""CPU: the fine-level refinement's oracle, fixture, pixel conversion, weight loading and argument checks.

tests/golden/fine_match*.npz holds what the reference's FinePreprocess, loftr_fine and FineMatching give
in float64 on the cases of tests/fine_oracle.py (recorded by tests/golden/make_fine_match.py). The oracle
is the definition in csrc/fine_match.hip's header restated in float64: it must reproduce the modules to
rounding."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fine_oracle as O


@pytest.fixture(scope="module")
def golden(golden_dir):
    return O.load_golden(golden_dir)


def _inputs(golden, case):
    return tuple(golden[f"{case}_{k}"] for k in ("fine_a", "fine_b", "coarse_a", "coarse_b"))


def _coarse(case, conf=None):
    from bundlesdf_amd.matching import CoarseMatches
    c = O.CASES[case]
    _, _, _, j_of_i = O.case_matches(case)
    j = torch.from_numpy(j_of_i)
    cf = torch.where(j >= 0, torch.full(j.shape, 0.5), torch.zeros(j.shape)) if conf is None else conf
    return CoarseMatches(j_of_i=j, conf=cf, n_matches=(j >= 0).sum(1).to(torch.int32), hw_a=c["hw_a"], hw_b=c["hw_b"])


@pytest.mark.parametrize("case", list(O.CASES))
def test_oracle_reproduces_the_reference_modules(golden, case):
    """Two float64 evaluations of one formula: the bound is 1e-9 absolute."""
    c = O.CASES[case]
    assert sum(len(d) for d in O.CASES["s4"]["matches"].values()) == 37
    inputs = _inputs(golden, case)
    for got, k in zip(O.make_inputs(case, float(golden[f"{case}_gain"])), ("fine_a", "fine_b", "coarse_a", "coarse_b")):
        np.testing.assert_array_equal(got, golden[f"{case}_{k}"])          # the stored inputs are the seeded ones
    out = O.refine(O.make_weights(c["seed"]), case, *inputs)
    for k, key in (("win_a", "win_a"), ("win_b", "win_b"), ("expec", "expec_f"), ("mkpts1_f", "mkpts1_f")):
        assert out[k].shape == golden[f"{case}_{key}"].shape
        assert np.abs(out[k] - golden[f"{case}_{key}"]).max() <= 1e-9, k
    # the conditions the maker asserted: heat maps neither flat nor saturated, the reference's own fp16 error far below
    assert float(golden[f"{case}_xy_rms"]) >= 0.1
    assert float(golden[f"{case}_xy_e16_max"]) < float(golden[f"{case}_xy_rms"]) / 20


def test_fixture_sees_axis_order_offset_and_centre_row(golden):
    """A transposed window, a window off by one and another centre row each miss the fixture by far more
    than the reference's own half-precision error."""
    case, c = "s4", O.CASES["s4"]
    w = O.make_weights(c["seed"])
    fa, fb, ca, cb = _inputs(golden, case)
    pair, i, j, _ = O.case_matches(case)
    good = O.refine(w, case, fa, fb, ca, cb)
    e_win, e_xy = float(golden[f"{case}_win_e16_max"]), float(golden[f"{case}_xy_e16_max"])
    t = good["win_a"].reshape(-1, 5, 5, O.C).transpose(0, 2, 1, 3).reshape(-1, 25, O.C)
    assert np.abs(t - golden[f"{case}_win_a"]).max() > 100 * e_win
    shifted = O.preprocess(w, np.roll(fa, 1, axis=3), ca, c["frames_a"], pair, i, c["hw_a"][1], c["stride"])
    assert np.abs(shifted - golden[f"{case}_win_a"]).max() > 100 * e_win
    f0 = good["f0"].copy()
    f0[:, 12] = good["f0"][:, 11]
    assert np.abs(O.expectation(f0, good["f1"])[:, :2] - golden[f"{case}_expec_f"][:, :2]).max() > 20 * e_xy


def test_corner_window_by_plain_slicing(golden):
    """The window of A's cell 0 (top left) and of its last cell, against slices of the map."""
    case, c = "s4", O.CASES["s4"]
    fa = golden[f"{case}_fine_a"]
    win = O.fine_windows(fa, np.array([0, 0]), np.array([0, 41]), c["hw_a"][1], c["stride"]).reshape(2, 5, 5, O.C)
    assert not win[0, :2].any() and not win[0, :, :2].any()                 # two rows and columns of padding
    np.testing.assert_array_equal(win[0, 2:, 2:], fa[0, :, 0:3, 0:3].transpose(1, 2, 0))
    y, x = 4 * 5, 4 * 6                                                     # cell 41 = (5, 6) of the 6 x 7 grid, map 24 x 28
    np.testing.assert_array_equal(win[1], fa[0, :, y - 2:y + 3, x - 2:x + 3].transpose(1, 2, 0))
    assert win[1].any(axis=2).all()                                         # stride 4: the last cell's window lies inside


def _fine_matches(case, expec):
    from bundlesdf_amd.fine import FineMatches
    c = O.CASES[case]
    pair, i, j, j_of_i = O.case_matches(case)
    counts = (j_of_i >= 0).sum(1)
    return FineMatches(pair=torch.from_numpy(pair), i=torch.from_numpy(i), j=torch.from_numpy(j),
                       conf=torch.full((len(pair),), 0.5), expec=torch.from_numpy(expec.astype(np.float32)),
                       pair_start=torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)),
                       hw_a=c["hw_a"], hw_b=c["hw_b"], stride=c["stride"])


def test_to_pixels_with_zero_expec_is_the_coarse_result():
    cm = _coarse("s4")
    M = 37
    rng = np.random.default_rng(3)
    tf = np.tile(np.eye(3), (3, 1, 1))
    tf[:, :2, :2] *= rng.uniform(0.5, 2.0, (3, 1, 1))
    tf[:, :2, 2] = rng.uniform(-20, 20, (3, 2))
    fm = _fine_matches("s4", np.zeros((M, 3)))
    for kw in (dict(), dict(tf_a=tf, tf_b=tf), dict(scale=4, tf_b=tf[0])):
        want = cm.to_pixels(**kw)
        got = fm.to_pixels(**kw)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and torch.equal(g, w)


def test_to_pixels_adds_the_expectation_before_the_inverse_transform(golden):
    case = "s4"
    pair, i, j, _ = O.case_matches(case)
    expec = golden[f"{case}_expec_f"].astype(np.float32)
    fm = _fine_matches(case, expec)
    cm = _coarse(case)
    uv_a, uv_b, ps, conf = fm.to_pixels(rounded=False)
    assert uv_b.dtype == torch.float64 and torch.equal(uv_a, cm.to_pixels()[0]) and torch.equal(ps, cm.to_pixels()[2])
    want = O.fine_pixels(j, 8, expec.astype(np.float64), 8)
    np.testing.assert_array_equal(uv_b.numpy(), want)
    assert np.abs(want - golden[f"{case}_mkpts1_f"]).max() < 1e-5          # float32 expec against the reference's float64
    r = fm.to_pixels()[1].numpy()
    np.testing.assert_array_equal(r, np.sign(want) * np.floor(np.abs(want) + 0.5))
    assert (r != cm.to_pixels()[1].numpy()).any()                           # offsets of up to 4 pixels do move pixels
    # with a transform: the offset is added in the descriptor image's frame, then the inverse is applied
    tf = np.array([[2.0, 0.0, 10.0], [0.0, 2.0, -6.0], [0.0, 0.0, 1.0]])
    got = fm.to_pixels(tf_b=tf, rounded=False)[1].numpy()
    np.testing.assert_allclose(got, (want - np.array([10.0, -6.0])) / 2.0, rtol=0, atol=1e-12)
    assert torch.equal(fm.to_pixels(tf_b=tf, rounded=False)[0], cm.to_pixels()[0])
    s4 = fm.to_pixels(scale=8, scale_f=4, rounded=False)[1].numpy()
    np.testing.assert_array_equal(s4, O.fine_pixels(j, 8, expec.astype(np.float64), 8, scale_f=4))
    with pytest.raises(ValueError, match="tf_b"):
        fm.to_pixels(tf_b=np.eye(4))


def test_from_state_dict_prefixes_packing_and_rejections():
    import bundlesdf_amd
    F = bundlesdf_amd.fine                                                  # exported as matching and transformer are
    from bundlesdf_amd import transformer as T
    w = O.make_weights(5)
    plain = F.FineRefiner(w)
    assert plain.packed.dtype == np.uint8 and plain.packed.size == F.WEIGHT_BYTES == 132096
    assert plain.transformer.d_model == 128 and plain.transformer.layer_names == ("self", "cross")
    for prefix in ("", "matcher."):
        sd = {prefix + k: torch.from_numpy(v) for k, v in w.items()}
        sd[prefix + "backbone.conv1.weight"] = torch.zeros(4, 4)
        sd.update({prefix + "loftr_coarse." + k: torch.from_numpy(v) for k, v in O.TO.make_weights(6, 256, ("self",)).items()})
        for given in (None, prefix):
            r = F.FineRefiner.from_state_dict(sd, prefix=given)
            np.testing.assert_array_equal(r.packed, plain.packed)
            np.testing.assert_array_equal(r.transformer.packed, plain.transformer.packed)
    # the packed block: down_proj, merge_feat's fine half, its context half (fragment order), the two biases
    wd = plain.packed[:65536].view(np.float16).reshape(4, 16, 64, 8)
    wf = plain.packed[65536:98304].view(np.float16).reshape(4, 8, 64, 8)
    wc = plain.packed[98304:131072].view(np.float16).reshape(4, 8, 64, 8)
    for nt, ks, lane, jj in ((0, 0, 0, 0), (3, 7, 63, 7), (1, 2, 37, 5)):
        row, col = 32 * nt + lane % 32, 16 * ks + 8 * (lane // 32) + jj
        assert wd[nt, ks, lane, jj] == w["fine_preprocess.down_proj.weight"][row, col]
        assert wd[nt, ks + 8, lane, jj] == w["fine_preprocess.down_proj.weight"][row, col + 128]
        assert wf[nt, ks, lane, jj] == w["fine_preprocess.merge_feat.weight"][row, col]
        assert wc[nt, ks, lane, jj] == w["fine_preprocess.merge_feat.weight"][row, 128 + col]
    bias = plain.packed[131072:].view(np.float32).reshape(2, 128)
    np.testing.assert_array_equal(bias[0], w["fine_preprocess.down_proj.bias"])
    np.testing.assert_array_equal(bias[1], w["fine_preprocess.merge_feat.bias"])
    np.testing.assert_array_equal(T.pack_matrix(w["fine_preprocess.down_proj.weight"].astype(np.float16)).reshape(4, 16, 64, 8), wd)

    for key in ("fine_preprocess.down_proj.weight", "fine_preprocess.down_proj.bias", "fine_preprocess.merge_feat.weight",
                "fine_preprocess.merge_feat.bias", "loftr_fine.layers.1.merge.weight"):
        missing = dict(w)
        del missing[key]
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            F.FineRefiner.from_state_dict(missing, prefix="")
        bad = dict(w)
        bad[key] = np.zeros((3, 3), np.float32)
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            F.FineRefiner.from_state_dict(bad, prefix="")
    with pytest.raises(ValueError, match="missing under every prefix"):
        F.FineRefiner.from_state_dict({"loftr_fine." + k: v for k, v in O.TO.make_weights(6, 128, ("self",)).items()})
    two = dict(w)
    two.update({"other." + k: v for k, v in w.items()})
    with pytest.raises(ValueError, match="name one"):
        F.FineRefiner.from_state_dict(two)
    with pytest.raises(ValueError, match="full"):
        F.FineRefiner(w, layer_names=("self", "full"))


def test_refine_rejects_bad_shapes_before_the_library_is_needed(golden, monkeypatch):
    from bundlesdf_amd import _lib, fine as F

    def no_library():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(_lib, "lib", no_library)
    case, c = "s4", O.CASES["s4"]
    r = F.FineRefiner(O.make_weights(c["seed"]))
    fa, fb, ca, cb = (torch.from_numpy(x).float() for x in _inputs(golden, case))
    cm = _coarse(case)
    ok = dict(fine_a=fa, fine_b=fb, coarse_a=ca, coarse_b=cb, frames_a=c["frames_a"], frames_b=c["frames_b"])

    def bad(match, cm_=cm, **kw):
        with pytest.raises(ValueError, match=match):
            r.refine(cm_, **{**ok, **kw})

    bad("CoarseMatches", cm_=(1, 2))
    bad("fine_a", fine_a=fa[0])                                             # not 4-d
    bad("fine_a", fine_a=fa.long())
    bad("fine_b.*128 channels", fine_b=fb[:, :64])
    bad("fine_a.*128 channels", fine_a=fa.half(), channels_last=True)       # channels first taken as channels last
    bad("fine_a is 23x28", fine_a=fa[:, :, :23])                            # hf is no multiple of h0
    bad("fine_b is 20x31", fine_b=fb[:, :, :, :31])
    bad("stride 2 and fine_b stride 4", fine_a=fa[:, :, :12, :14])
    bad("coarse_a", coarse_a=ca[:, :41])
    bad("coarse_b", coarse_b=cb[:2])
    bad("coarse_b", coarse_b=cb[:, :, :128])
    bad("frames_a", frames_a=(0, 1))
    bad("frames_a", frames_a=(0, 1, 3))                                     # 3 maps: 0 .. 2
    bad("frames_b", frames_b=(0.0, 1.0, 2.0))
    bad("give frames_a", fine_a=fa[:2], frames_a=None)                      # 2 maps for 3 pairs
    bad("chunk", chunk=0)
    from bundlesdf_amd.matching import CoarseMatches
    bad("hw_a", cm_=CoarseMatches(j_of_i=cm.j_of_i, conf=cm.conf, n_matches=cm.n_matches, hw_a=(6, 6), hw_b=(5, 8)))


def test_entry_points_refuse_bad_descriptors_before_device_work():
    """NOF_EINVAL with the field named, on a machine with no GPU: the descriptors are validated before the
    first HIP call."""
    from bundlesdf_amd import _lib, build
    build.build()
    lib = _lib.lib()
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def wdesc(**kw):
        D = _lib.FineWindowsDesc()
        D.M, D.P, D.N_a, D.N_b, D.h0, D.w0, D.h1, D.w1, D.stride = 37, 3, 3, 3, 6, 7, 5, 8, 4
        D.pair = D.i = D.j = p
        D.weights_bytes = 132096
        for k, v in kw.items():
            setattr(D, k, v)
        return D

    for kw, text in ((dict(M=-1), b"M=-1"), (dict(M=(1 << 24) + 1), b"M=16777217"), (dict(P=0), b"P=0"),
                     (dict(pair=None), b"pair is NULL"), (dict(j=None), b"j is NULL"), (dict(N_a=0), b"N_a=0"),
                     (dict(N_b=-2), b"N_b=-2"), (dict(stride=0), b"stride=0"), (dict(h0=0), b"h0=0"), (dict(w1=0), b"w1=0"),
                     (dict(h1=8193), b"stride h1=32772"), (dict(weights_bytes=132095), b"weights_bytes=132095"),
                     (dict(), b"fine_a is NULL"), (dict(fine_a=p), b"fine_b is NULL"),
                     (dict(fine_a=p + 8), b"fine_a must be 16-byte aligned"),
                     (dict(fine_a=p, fine_b=p, coarse_a=p, coarse_b=p, weights=p, context=p, win_a=p), b"win_b is NULL"),
                     (dict(M=0), b"fine_a is NULL")):
        assert lib.nof_fine_windows(ctypes.byref(wdesc(**kw)), None) == 1, kw
        assert text in lib.nof_last_error(), (kw, lib.nof_last_error())
    assert lib.nof_fine_windows(None, None) == 1 and b"desc is NULL" in lib.nof_last_error()
    # a whole descriptor with no match: NOF_OK, and nothing is launched
    assert lib.nof_fine_windows(ctypes.byref(wdesc(M=0, fine_a=p, fine_b=p, coarse_a=p, coarse_b=p, weights=p, context=p,
                                                   win_a=p, win_b=p, pair=None, i=None, j=None)), None) == 0

    def edesc(**kw):
        D = _lib.FineExpectationDesc()
        D.M, D.P, D.L, D.S = 37, 3, 42, 40
        D.pair = D.i = D.j = p
        for k, v in kw.items():
            setattr(D, k, v)
        return D

    for kw, text in ((dict(M=-5), b"M=-5"), (dict(P=0), b"P=0"), (dict(i=None), b"i is NULL"), (dict(L=0), b"L=0"),
                     (dict(S=0), b"S=0"), (dict(), b"win_a is NULL"), (dict(win_a=p, win_b=p), b"expec is NULL"),
                     (dict(win_a=p, win_b=p + 4, expec=p), b"16-byte aligned")):
        assert lib.nof_fine_expectation(ctypes.byref(edesc(**kw)), None) == 1, kw
        assert text in lib.nof_last_error(), (kw, lib.nof_last_error())
    assert lib.nof_fine_expectation(ctypes.byref(edesc(M=0, win_a=p, win_b=p, expec=p)), None) == 0


def test_forward_inplace_rejects_what_it_cannot_update_in_place():
    from bundlesdf_amd import transformer as T
    ft = T.FeatureTransformer(O.TO.make_weights(3, 128, ("self",)), d_model=128, layer_names=("self",))
    a, b = torch.zeros(2, 25, 128), torch.zeros(2, 25, 128)
    for xa, xb, text in ((a.half(), b, "float32"), (a[:, ::2], b, "contiguous"), (a, b[:1], "P and C"),
                         (torch.zeros(2, 25, 256), torch.zeros(2, 25, 256), "d_model=128"), (a, b, "one device")):
        with pytest.raises(ValueError, match=text):
            ft.forward_inplace(xa, xb)
