"""GPU: nof_backbone against the reference's ResNetFPN_8_2, its determinism, its input forms and the chain
from images to refined matches.

Parity bound. tests/golden/backbone*.npz holds the module's float64 outputs and its own half-precision
error e16 (fp16 autocast minus float64, rms and max per output). The device rounds at other points than
autocast (folded weights, every stored activation), so it is held to 2 x e16, rms and max, per case and per
output: the project's standing bound for such kernels (test_gpu_transformer.py, test_gpu_fine.py)."""
import numpy as np
import pytest
import torch

from tests import backbone_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return O.load_golden(golden_dir)


@pytest.fixture(scope="module")
def net(cuda_device):
    from bundlesdf_amd.backbone import Backbone
    return Backbone(O.make_weights(), device=cuda_device)


@pytest.fixture(scope="module")
def outputs(net, cuda_device):
    """case -> (images on the device, coarse without pe, fine, hw), computed once and left unchanged."""
    out = {}
    for case in O.CASES:
        x = torch.from_numpy(O.make_images(case)).to(cuda_device)
        coarse, fine, hw = net.forward(x, position_encoding=False)
        out[case] = (x, coarse, fine, hw)
    return out


@pytest.mark.parametrize("case", list(O.CASES))
def test_parity_with_the_reference_module(outputs, golden, case):
    c = O.CASES[case]
    _, coarse, fine, hw = outputs[case]
    hc, wc = c["H"] // 8, c["W"] // 8
    assert hw == (hc, wc)
    assert coarse.dtype == torch.float32 and tuple(coarse.shape) == (c["N"], hc * wc, 256)
    assert fine.dtype == torch.float16 and tuple(fine.shape) == (c["N"], c["H"] // 2, c["W"] // 2, 128)
    assert torch.isfinite(coarse).all() and torch.isfinite(fine).all()
    got = {"coarse": coarse.double().cpu().numpy().reshape(c["N"], hc, wc, 256).transpose(0, 3, 1, 2),
           "fine": fine.double().cpu().numpy().transpose(0, 3, 1, 2)}
    ratios = {}
    for key in ("coarse", "fine"):
        err = got[key] - golden[f"{case}_{key}64"]
        rms, mx = float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())
        e_rms, e_max = float(golden[f"{case}_{key}_e16_rms"]), float(golden[f"{case}_{key}_e16_max"])
        ratios[key] = (rms, e_rms, mx, e_max)
        print(f"{case} {key}: rms {rms:.3e} = {rms / e_rms:.2f} e16_rms, max {mx:.3e} = {mx / e_max:.2f} e16_max")
    for key, (rms, e_rms, mx, e_max) in ratios.items():
        assert rms <= 2 * e_rms, (case, key, rms, e_rms)
        assert mx <= 2 * e_max, (case, key, mx, e_max)


def test_same_bytes_on_every_call_and_for_every_split(net, outputs):
    x, coarse, fine, _ = outputs["ragged"]
    again = net.forward(x, position_encoding=False)
    assert torch.equal(again[0], coarse) and torch.equal(again[1], fine)
    for n in range(x.shape[0]):
        one = net.forward(x[n:n + 1], position_encoding=False)
        assert torch.equal(one[0], coarse[n:n + 1]) and torch.equal(one[1], fine[n:n + 1]), n


@pytest.mark.parametrize("fix", [False, True])
def test_fused_position_encoding_equals_the_sum_in_torch(net, outputs, fix):
    from bundlesdf_amd.transformer import position_encoding
    x, coarse, fine, (hc, wc) = outputs["ragged"]
    tok, fine_pe, _ = net.forward(x, temp_bug_fix=fix)
    assert torch.equal(tok, coarse + position_encoding(hc, wc, 256, fix, device=coarse.device)[None])
    assert torch.equal(fine_pe, fine) and not torch.equal(tok, coarse)


def test_input_forms_give_the_same_bytes(net, outputs):
    x, coarse, fine, _ = outputs["wide"]                    # fp16 values: exact in every float dtype
    for form in (x[:, None], x.cpu().numpy(), x.half(), x.double(), x.cpu().numpy().astype(np.float64)[:, None]):
        c2, f2, _ = net.forward(form, position_encoding=False)
        assert c2.is_cuda and torch.equal(c2, coarse) and torch.equal(f2, fine)


def test_no_trace_of_the_pad_channels(net, cuda_device):
    """Every 196-channel activation is stored with 28 pad channels. With the scratch buffer full of NaN
    bytes before the call (a pad channel that the kernels did not write as 0 would be read as NaN by the
    next layer) the outputs are what they were."""
    x = torch.from_numpy(O.make_images("wide")).to(cuda_device)
    clean = net.forward(x, position_encoding=False)
    net._scratch[clean[0].device].fill_(0xff)
    dirty = net.forward(x, position_encoding=False)
    assert torch.isfinite(dirty[0]).all() and torch.isfinite(dirty[1]).all()
    assert torch.equal(dirty[0], clean[0]) and torch.equal(dirty[1], clean[1])
    assert tuple(dirty[0].shape) == (1, 3 * 9, 256) and tuple(dirty[1].shape) == (1, 12, 36, 128)


# ---- exact integer runs and one-layer bounds (profiles/r25/backbone_layerwise.md) ----
#
# The parity bound above spans 20 layers and two networks that round at different points; a slip the size of
# one fp16 rounding passes it. Below nothing is end to end: under tests/backbone_oracle.exact_weights every
# product, partial sum and stored activation is an integer that fp16 and float32 hold exactly, so the
# device must equal the float64 oracle with no tolerance; and the layers whose input and output both
# survive in the scratch buffer are checked alone from the device's own input, to a bound derived from the
# number formats (O.layer_bound).

EXACT_CASES = ("ragged", "one_cell")
ISOLATED = {13: ("c0", "c1"), 16: ("m2", "m1"), 17: ("s0", "s1"), 18: ("s1", "s2"), 19: ("s2", "fine")}   # layer -> (input, output)


def _forward_snapshot(net, x, poison=False):
    """One call -> (coarse [N,hc,wc,256] f32, fine f16, the nine scratch tensors), numpy copies taken before
    anything else runs. poison: the scratch buffer holds 0xff bytes (fp16 NaN) when the call starts."""
    N, H, W = x.shape
    if poison:
        if x.device not in net._scratch:
            net.forward(x, position_encoding=False)
        net._scratch[x.device].fill_(0xff)
    coarse, fine, (hc, wc) = net.forward(x, position_encoding=False)
    views = O.scratch_views(net._scratch[x.device], N, H, W)
    snap = {k: v.cpu().numpy() for k, v in views.items()}
    snap["coarse"] = coarse.cpu().numpy().reshape(N, hc, wc, 256)
    snap["fine"] = fine.cpu().numpy()
    return snap


@pytest.fixture(scope="module")
def exact_runs(cuda_device):
    """(kind, case) -> (snapshot of the device's call on poisoned scratch, the oracle's trace), computed once."""
    from bundlesdf_amd.backbone import Backbone
    dev = torch.device(cuda_device)
    dev = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
    out = {"dev": dev}
    for kind in ("trunk", "head"):
        w = O.exact_weights(kind)
        out[kind] = net = Backbone(w, device=dev)
        for case in EXACT_CASES:
            images = O.exact_images(case)
            trace = {}
            O.forward(w, images, rounded=True, trace=trace)
            out[kind, case] = (_forward_snapshot(net, torch.from_numpy(images).to(dev), poison=True), trace)
    return out


def _assert_holds(snap, trace, part):
    """The scratch part equals the oracle's activation in its real channels and is 0 in its pad channels."""
    want = trace[O.SCRATCH_HOLDS[part]]
    C = want.shape[-1]
    got = snap[part].astype(np.float64)
    np.testing.assert_array_equal(got[..., :C], want, err_msg=part)
    np.testing.assert_array_equal(got[..., C:], 0.0, err_msg=part + " pad channels")   # NaN where nobody wrote


@pytest.mark.parametrize("case", EXACT_CASES)
def test_exact_trunk_equals_the_oracle_bit_for_bit(exact_runs, case):
    """Stem, the six BasicBlocks (stride 2 and the fused skip included) and layer3_outconv, no tolerance."""
    snap, trace = exact_runs["trunk", case]
    for part in ("s0", "m0", "c0", "c2", "c1"):
        _assert_holds(snap, trace, part)
    assert snap["m0"].shape[-1] == 224 and trace[O.SCRATCH_HOLDS["m0"]].shape[-1] == 196      # 28 pad channels
    assert snap["coarse"].dtype == np.float32
    np.testing.assert_array_equal(snap["coarse"].astype(np.float64), trace["coarse"])

    # N = 2 in one call and in two calls
    net, dev = exact_runs["trunk"], exact_runs["dev"]
    x = torch.from_numpy(O.exact_images(case)).to(dev)
    x = x if x.shape[0] == 2 else torch.cat([x, x.flip(2)])
    both = _forward_snapshot(net, x)
    if case == "ragged":
        for key in both:
            np.testing.assert_array_equal(both[key], snap[key], err_msg=key)
    for n in range(2):
        one = _forward_snapshot(net, x[n:n + 1])
        for key in ("s0", "m0", "c0", "c2", "c1", "coarse", "fine"):
            np.testing.assert_array_equal(one[key], both[key][n:n + 1], err_msg=f"{key} image {n}")


@pytest.mark.parametrize("case", EXACT_CASES)
def test_exact_head_equals_the_oracle_bit_for_bit(exact_runs, case):
    """layer3_outconv and layer2_outconv2.3 zero: both up2 terms are 0, and layer2_outconv (through
    layer2_outconv2.0, whose input it is), layer2_outconv2.0, layer1_outconv and layer1_outconv2.0 are exact;
    lrelu's negative branch is one float32 product rounded to fp16."""
    snap, trace = exact_runs["head", case]
    for part in ("m2", "s1", "s2", "s0", "m0", "c0"):
        _assert_holds(snap, trace, part)
    assert snap["s1"].shape[-1] == snap["s2"].shape[-1] == 224
    for part in ("m1", "c1", "coarse"):
        np.testing.assert_array_equal(snap[part], 0.0, err_msg=part)


@pytest.fixture(scope="module")
def isolated(net, cuda_device):
    """case -> snapshot of the device's call with the random weights (the scratch buffer is shared between the
    cases, so each is copied right after its call)."""
    dev = torch.device(cuda_device)
    dev = dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())
    return {case: _forward_snapshot(net, torch.from_numpy(O.make_images(case)).to(dev)) for case in O.CASES}


@pytest.fixture(scope="module")
def random_weights():
    return O.make_weights()


@pytest.mark.parametrize("li", sorted(ISOLATED))
@pytest.mark.parametrize("case", list(O.CASES))
def test_one_layer_from_the_devices_own_input(isolated, random_weights, case, li):
    """|got - ref| <= 2^-11 max(|got|, |ref|) + 2^-24 + (K + 8) 2^-23 A for every element: half an fp16 ulp
    (normal, subnormal) for the one rounding of the store, and a float32 sum of K exact products in any order
    with the epilogue's few operations, A = sum |w||x| + |b'| + |res| + |up taps|. Derived, not tuned."""
    snap = isolated[case]
    src, dst = ISOLATED[li]
    ref, A = O.layer_reference(random_weights, li, snap[src], up=snap["m1"] if li == 17 else None)
    C = ref.shape[-1]
    got = snap[dst].astype(np.float64)
    assert np.isfinite(got).all() and np.abs(ref).max() > 0.1
    err = np.abs(got[..., :C] - ref)
    ratio = err / O.layer_bound(li, got[..., :C], ref, A)
    print(f"layer {li} {case}: max err {err.max():.3e}, max err / bound {ratio.max():.3f}")
    assert (ratio <= 1.0).all(), (case, li, float(ratio.max()))
    np.testing.assert_array_equal(got[..., C:], 0.0)
    if li == 13:
        coarse = snap["coarse"]
        r32 = np.abs(coarse.astype(np.float64) - ref) / O.layer_bound(li, coarse, ref, A, half=False)
        print(f"layer 13 {case} coarse: max err / bound {r32.max():.3f}")
        assert (r32 <= 1.0).all(), (case, float(r32.max()))
        np.testing.assert_array_equal(snap["c1"].view(np.uint16), coarse.astype(np.float16).view(np.uint16))


def test_float32_images_are_rounded_to_fp16_to_nearest_even(net, cuda_device):
    """The stem rounds the image when it stages it: a float32 image gives the bytes of that image rounded to
    fp16 on the host. 1 + 2^-11 lies half-way between 1 and 1 + 2^-10 and goes down to the even 1;
    1 + 3 2^-11 lies half-way between 1 + 2^-10 and 1 + 2^-9 and goes up to the even 1 + 2^-9."""
    rng = np.random.default_rng(77)
    x = rng.random((2, 16, 24)).astype(np.float32)
    lo, hi = np.float32(1 + 2.0 ** -11), np.float32(1 + 3 * 2.0 ** -11)
    x[:, ::3, ::5], x[:, 1::3, 2::5] = lo, hi
    x16 = x.astype(np.float16)
    assert float(np.float16(lo)) == 1.0 < lo and float(np.float16(hi)) == 1 + 2.0 ** -9 > hi
    assert (x16.astype(np.float32) != x).mean() > 0.9
    want = net.forward(torch.from_numpy(x16.astype(np.float32)).to(cuda_device), position_encoding=False)
    got = net.forward(torch.from_numpy(x).to(cuda_device), position_encoding=False)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # the two half-way values matter: rounding them the other way changes the output
    other = x16.copy()
    other[:, ::3, ::5], other[:, 1::3, 2::5] = np.float16(1 + 2.0 ** -10), np.float16(1 + 2.0 ** -10)
    moved = net.forward(torch.from_numpy(other.astype(np.float32)).to(cuda_device), position_encoding=False)
    assert not torch.equal(moved[1], want[1])


def _scene_images(dev):
    """Two renders of the shared synthetic mesh at 96 x 128 -> (rgb uint8 [2,96,128,3], grey [2,96,128] f32)."""
    from bundlesdf_amd.compat.loftr_wrapper import to_grey
    from bundlesdf_amd.mesh_render import MeshRenderer
    from tests import mesh_render_oracle as MR
    s = MR.scene()
    K = np.array([[120.0, 0.0, 63.5], [0.0, 120.0, 47.5], [0.0, 0.0, 1.0]])
    r = MeshRenderer(s["mesh"], K, 96, 128, znear=MR.ZNEAR, zfar=MR.ZFAR, device=dev)
    rgb = r.render(np.array(s["poses"][:2]), colour="vertex")["rgb"].cpu().numpy()
    return rgb, to_grey(rgb)


def _matcher_weights():
    from tests import fine_oracle as FO
    w = {"backbone." + k: v for k, v in O.make_weights().items()}
    w.update({"loftr_coarse." + k: v for k, v in FO.TO.make_weights(41, 256, ("self", "cross") * 4).items()})
    w.update(FO.make_weights(42))
    return {"matcher." + k: torch.from_numpy(v) for k, v in w.items()}


def test_loftr_match_equals_the_stages_called_by_hand(cuda_device):
    from bundlesdf_amd.compat.loftr_wrapper import LoftrRunner
    from bundlesdf_amd.loftr import Loftr
    from bundlesdf_amd.matching import match_descriptors
    dev = cuda_device
    rgb, grey = _scene_images(dev)
    assert grey.std() > 0.05                                           # the renders are not blank
    sd = _matcher_weights()
    m = Loftr.from_state_dict(sd, device=dev)
    pairs = np.array([(0, 1), (1, 0)])
    fm = m.match(grey, pairs, thr=0.0, border_rm=0)

    tok, fine, hw = m.backbone.forward(grey)
    assert hw == (12, 16)
    da, db = m.coarse.forward(tok[pairs[:, 0]], tok[pairs[:, 1]])
    cm = match_descriptors(da, db, hw, hw, thr=0.0, border_rm=0)
    want = m.refiner.refine(cm, fine, fine, da, db, frames_a=pairs[:, 0], frames_b=pairs[:, 1])
    assert want.expec.shape[0] > 0
    for name in ("pair", "i", "j", "conf", "expec", "pair_start"):
        assert torch.equal(getattr(fm, name), getattr(want, name)), name
    assert (fm.hw_a, fm.hw_b, fm.stride) == (want.hw_a, want.hw_b, want.stride) == (hw, hw, 4)
    # a frame that is in no pair is not run, and the pairs are renumbered
    three = np.concatenate([grey[:1], np.zeros_like(grey[:1]), grey[1:]])
    far = m.match(three, np.array([(0, 2), (2, 0)]), thr=0.0, border_rm=0)
    assert torch.equal(far.expec, fm.expec) and torch.equal(far.j, fm.j)

    runner = LoftrRunner({"state_dict": sd}, device=dev, thr=0.0)
    out = runner.predict(rgb[:1], rgb[1:])
    one = runner.matcher.match(grey, np.array([(0, 1)]), thr=0.0)
    uv_a, uv_b, _, conf = one.to_pixels(rounded=False)
    assert len(out) == 1 and out[0].dtype == np.float32 and out[0].shape == (uv_a.shape[0], 5)
    np.testing.assert_array_equal(out[0][:, 0:2], uv_a.cpu().numpy().astype(np.float32))
    np.testing.assert_array_equal(out[0][:, 2:4], uv_b.cpu().numpy().astype(np.float32))
    np.testing.assert_array_equal(out[0][:, 4], conf.cpu().numpy())
