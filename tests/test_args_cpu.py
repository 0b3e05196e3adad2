"""bundlesdf_amd/_args.py: the argument, device and weight plumbing of the wrappers, each helper on its own."""
import numpy as np
import pytest
import torch

from bundlesdf_amd import _args as A


def test_as_tensor_copies_arrays_and_leaves_tensors_alone():
    ro = np.arange(6, dtype=np.float32).reshape(2, 3)
    ro.setflags(write=False)
    t = A.as_tensor(ro)
    t[0, 0] = 7.0                                            # writable, and not the caller's memory
    assert ro[0, 0] == 0.0 and t.dtype == torch.float32 and tuple(t.shape) == (2, 3)
    assert A.as_tensor([[1, 2], [3, 4]], np.float64).dtype == torch.float64
    for x in (torch.zeros(3, dtype=torch.int16), torch.zeros(2, 2, dtype=torch.float16, device="meta")):
        y = A.as_tensor(x, np.float64)                       # a tensor keeps its dtype and its device
        assert y.dtype == x.dtype and y.device == x.device and y.data_ptr() == x.data_ptr()
    g = torch.ones(4, requires_grad=True)
    assert not A.as_tensor(g * 2).requires_grad and not A.as_tensor(g).requires_grad


def test_as_host_is_contiguous_of_the_dtype_and_a_copy():
    base = np.arange(24, dtype=np.int32).reshape(4, 6)
    for a in (torch.arange(6, dtype=torch.float32).reshape(2, 3).t(), [[1, 2, 3], [4, 5, 6]], base[:, ::2], base.T,
              (torch.ones(3, requires_grad=True) * 2)):
        h = A.as_host(a, np.float64)
        assert isinstance(h, np.ndarray) and h.dtype == np.float64 and h.flags["C_CONTIGUOUS"] and h.flags["WRITEABLE"]
        np.testing.assert_array_equal(h, np.asarray(a.detach() if torch.is_tensor(a) else a, np.float64))
    assert A.as_host(base[:, ::2]).dtype == np.int32 and A.as_host(torch.zeros(2, dtype=torch.float16)).dtype == np.float16
    same = np.zeros(3)
    assert not np.shares_memory(A.as_host(same, np.float64), same)
    assert A.as_host(2.5, np.float64).reshape(-1).tolist() == [2.5]


def test_default_device(monkeypatch):
    asked = []

    def current():
        asked.append(1)
        return 3

    monkeypatch.setattr(torch.cuda, "current_device", current)
    assert A.default_device(device="cuda:1") == torch.device("cuda", 1) and not asked     # explicit, with an index
    assert A.default_device(torch.zeros(1), "cuda:1") == torch.device("cuda", 1) and not asked
    assert A.default_device(device="cpu") == torch.device("cpu") and not asked
    assert A.default_device(device=torch.device("cuda")) == torch.device("cuda", 3)        # always an index
    assert A.default_device(torch.zeros(1)) == torch.device("cuda", 3)                     # a host tensor
    assert A.default_device(np.zeros(1)) == torch.device("cuda", 3) == A.default_device()
    assert A.default_device().index == 3


def test_packed_weights_lookup_and_find_prefix():
    w = {"p.a.weight": np.zeros((2, 3), np.float32), "p.b": torch.ones(4, dtype=torch.float16)}
    v = A.PackedWeights.lookup(w, "p.", "a.weight", (2, 3), "Thing")
    assert v.dtype == np.float32 and v.shape == (2, 3)
    assert A.PackedWeights.lookup(w, "p.", "b", (4,), "Thing").dtype == np.float16        # a tensor, its own dtype
    with pytest.raises(ValueError) as e:
        A.PackedWeights.lookup(w, "q.", "a.weight", (2, 3), "Thing")
    assert str(e.value) == "Thing: key 'q.a.weight' is missing"
    with pytest.raises(ValueError) as e:
        A.PackedWeights.lookup(w, "p.", "a.weight", (3, 2), "Thing")
    assert str(e.value) == "Thing: key 'p.a.weight' has shape (2, 3), expected (3, 2)"

    probe = "a.weight"
    assert A.PackedWeights.find_prefix(w, probe, "Thing", "a thing") == "p."
    assert A.PackedWeights.find_prefix({probe: 0}, probe, "Thing", "a thing") == ""
    with pytest.raises(ValueError) as e:
        A.PackedWeights.find_prefix({"p.b": 0}, probe, "Thing", "a thing")
    assert str(e.value) == "Thing: key 'a.weight' is missing under every prefix"
    with pytest.raises(ValueError) as e:
        A.PackedWeights.find_prefix({"z." + probe: 0, "p." + probe: 0}, probe, "Thing", "a thing")
    assert str(e.value) == "Thing: prefixes ['p.', 'z.'] all hold a thing, name one"


def test_packed_weights_per_device_copies_and_buffer():
    cpu = torch.device("cpu")
    packed = np.arange(16, dtype=np.uint8)
    pw = A.PackedWeights(packed)
    assert pw.packed is packed and pw._weights == {} and pw._buffers == {}
    w = pw.device_weights("cpu")
    assert w.dtype == torch.uint8 and w.tolist() == packed.tolist() and pw.device_weights(cpu) is w
    assert list(A.PackedWeights(packed, device="cpu")._weights) == [cpu]                  # uploaded at construction
    b = pw.buffer(cpu, 100)
    assert b.dtype == torch.uint8 and b.numel() == 100 and pw.buffer(cpu, 40) is b and pw.buffer(cpu, 100) is b
    b2 = pw.buffer(cpu, 101)
    assert b2 is not b and b2.numel() == 101 and pw._buffers[cpu] is b2
    assert A.PackedWeights(packed).buffer(cpu, 0).numel() == 1                            # never an empty allocation


def _pixels_reference(cell, w, pair, scale, tf, offset, rounded):
    """The documented rule in numpy float64: (c % w, c // w) scale (+ offset), through the inverse of the pair's
    transform with the sum taken as (x + y) + z, then C round()."""
    xy = np.stack([cell % w, cell // w], 1).astype(np.float64) * float(scale)
    if offset is not None:
        xy = xy + offset
    if tf is not None:
        Ti = np.linalg.inv(np.broadcast_to(tf, (pair.max() + 1, 3, 3)) if tf.ndim == 2 else tf)[pair]
        q = (Ti[:, :, 0] * xy[:, 0:1] + Ti[:, :, 1] * xy[:, 1:2]) + Ti[:, :, 2]
        xy = q[:, :2] / q[:, 2:3]
    return np.sign(xy) * np.floor(np.abs(xy) + 0.5) if rounded else xy


def test_cells_to_pixels_against_the_formula_and_both_match_classes():
    from bundlesdf_amd.fine import WINDOW, FineMatches
    from bundlesdf_amd.matching import CoarseMatches
    h, w, P = 5, 7, 3
    # cells on the first and the last column of the 5 x 7 grid, and one inside; (pair, i) ascending
    pair = np.array([0, 0, 1, 1, 1, 2, 2], np.int64)
    i = np.array([0, 6, 7, 17, 34, 13, 28], np.int64)
    j = np.array([34, 0, 6, 20, 28, 14, 27], np.int64)
    assert set(i % w) >= {0, 6} and set(j % w) >= {0, 6}
    # triangular, powers of two on the diagonal: their inverses are exact, whichever routine forms them
    tf = np.array([[[2.0, 0.0, 3.0], [0.0, 4.0, -5.0], [0.0, 0.0, 1.0]],
                   [[0.5, 0.25, 1.0], [0.0, 2.0, 2.0], [0.0, 0.0, 1.0]],
                   [[1.0, -0.5, 2.0], [0.0, 0.25, -1.0], [0.0, 0.0, 2.0]]])
    expec = np.array([[0.5, -0.25], [-1.0, 1.0], [0.0, 0.0], [0.125, 0.5], [-0.5, -0.5], [1.0, -1.0], [0.25, 0.75]])
    offset = expec * float((WINDOW // 2) * 2)
    ti, tj, tp = torch.from_numpy(i), torch.from_numpy(j), torch.from_numpy(pair)
    for rounded in (True, False):
        for T in (None, tf[1], tf):
            for off in (None, offset):
                got = A.cells_to_pixels(tj, w, tp, P, 8, None if T is None else T.copy(), "tf_b",
                                        None if off is None else torch.from_numpy(off), rounded)
                want = _pixels_reference(j, w, pair, 8, T, off, rounded)
                assert got.dtype == torch.float64 and got.numpy().tobytes() == want.tobytes(), (rounded, T, off)
    half = A.cells_to_pixels(ti[:2], w, tp[:2], P, 1, None, "tf_a", torch.tensor([[0.5, -0.5], [-6.5, 2.5]], dtype=torch.float64))
    assert half.tolist() == [[1.0, -1.0], [-1.0, 3.0]]                                    # halves away from zero
    assert torch.equal(A.cells_to_pixels(ti, w, tp, P, 8, torch.from_numpy(tf).float(), "tf_a"),
                       A.cells_to_pixels(ti, w, tp, P, 8, tf.tolist(), "tf_a"))          # tensor, any dtype, or list
    for bad in (np.eye(4), np.tile(np.eye(3), (2, 1, 1))):
        with pytest.raises(ValueError) as e:
            A.cells_to_pixels(ti, w, tp, P, 8, bad, "tf_a")
        assert str(e.value) == f"to_pixels: tf_a must be [3,3] or [3,3,3], got {bad.shape}"

    # the two classes are this function: CoarseMatches.to_pixels, FineMatches.to_pixels (uv_a without, uv_b with the offset)
    j_of_i = np.full((P, h * w), -1, np.int32)
    j_of_i[pair, i] = j
    cm = CoarseMatches(j_of_i=torch.from_numpy(j_of_i), conf=torch.rand(P, h * w), n_matches=torch.zeros(P, dtype=torch.int32),
                       hw_a=(h, w), hw_b=(h, w))
    ua, ub, ps, conf = cm.to_pixels(scale=8, tf_a=tf, tf_b=tf[1])
    assert ua.numpy().tobytes() == _pixels_reference(i, w, pair, 8, tf, None, True).tobytes()
    assert ub.numpy().tobytes() == _pixels_reference(j, w, pair, 8, tf[1], None, True).tobytes()
    assert ps.tolist() == [0, 2, 5, 7] and torch.equal(conf, cm.conf[tp, ti])
    fm = FineMatches(pair=tp.int(), i=ti.int(), j=tj.int(), conf=conf, pair_start=ps, hw_a=(h, w), hw_b=(h, w), stride=4,
                     expec=torch.from_numpy(np.concatenate([expec, np.zeros((7, 1))], 1)).float())
    for rounded in (True, False):
        fa, fb, _, _ = fm.to_pixels(scale=8, scale_f=2, tf_a=tf, tf_b=tf, rounded=rounded)
        assert fa.numpy().tobytes() == _pixels_reference(i, w, pair, 8, tf, None, rounded).tobytes()
        assert fb.numpy().tobytes() == _pixels_reference(j, w, pair, 8, tf, offset, rounded).tobytes()
    assert torch.equal(fm.to_pixels(tf_a=tf)[0], ua)
