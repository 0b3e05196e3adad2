"""CPU: vertex colours from the training images (nof_vertex_color_accumulate,
texture.vertex_colors_from_images). The two restatements of tests/vertex_colour_oracle.py agree on the
fixture the GPU test uses, the fixture has no near ties, and what needs no device: the config key, the
C ABI's argument checks through the loaded library, and the counts on Mesh."""
import ctypes

import numpy as np
import pytest

from tests import vertex_colour_oracle as VC


@pytest.mark.parametrize("radius", VC.RADII)
def test_restatements_agree(radius):
    ref = VC.fixture_reference(radius)
    for (bn, bd), (kn, kd) in zip(ref["brute"], ref["kdtree"]):
        m = bn >= 0
        assert m.any() and not m.all()
        assert np.array_equal(m, kd <= radius)
        assert np.array_equal(bn[m], kn[m])
        assert np.all(np.abs(bd[m] - kd[m]) <= 1e-12 * kd[m])
    assert np.array_equal(ref["brute_count"], ref["kdtree_count"])
    assert np.array_equal(ref["brute_rgb"], ref["kdtree_rgb"])
    share, multi = np.mean(ref["brute_count"] > 0), np.mean(ref["brute_count"] > 1)
    print(f"radius {radius}: coloured share {share:.3f}, more than one frame {multi:.3f}")
    assert 0.25 <= share <= 0.8 and multi >= 0.05


def test_fixture_has_no_near_ties():
    """The cKDTree breaks ties its own way; nearest-index equality is only a fair check where the two
    nearest candidates of a vertex differ by more than rounding."""
    fx = VC.fixture()
    worst = np.inf
    for fr in fx["frames"]:
        d = VC.two_nearest(fx["V"], fr["pts"])
        worst = min(worst, float(((d[:, 1] - d[:, 0]) / d[:, 1]).min()))
    print(f"smallest relative gap between the two nearest candidates: {worst:.3e}")
    assert worst > 1e-6


def test_unknown_colour_source_refused():
    from bundlesdf_amd.nerf_runner import _check_supported
    _check_supported({})
    _check_supported({"mesh_vertex_color_source": "network"})
    _check_supported({"mesh_vertex_color_source": "train_images"})
    with pytest.raises(ValueError, match="mesh_vertex_color_source"):
        _check_supported({"mesh_vertex_color_source": "images"})


@pytest.fixture(scope="module")
def libnof():
    from bundlesdf_amd import build
    build.build()
    from bundlesdf_amd import _lib
    return _lib.lib()


def test_bad_arguments_refused_before_device_work(libnof):
    """NOF_EINVAL and the argument's name, on a machine with no GPU."""
    Hh, Ww, n = 4, 5, 3
    host = dict(zbuf=np.zeros(Hh * Ww, np.uint64), mask=np.ones(Hh * Ww, np.uint8),
                colors=np.zeros((Hh * Ww, 3), np.float32), cam_in_ob=np.eye(4), ob_in_cam=np.eye(4), K=np.eye(3),
                V=np.zeros((n, 3), np.float32), color_sum=np.zeros((n, 3)), count=np.zeros(n, np.int32))

    def call(radius=0.01, min_depth=0.1, H=Hh, W=Ww, n_vertices=n, **null):
        p = {k: (None if k in null else v.ctypes.data_as(ctypes.c_void_p)) for k, v in host.items()}
        return libnof.nof_vertex_color_accumulate(p["zbuf"], H, W, p["mask"], min_depth, p["colors"], p["cam_in_ob"],
                                                  p["ob_in_cam"], p["K"], p["V"], n_vertices, radius, p["color_sum"],
                                                  p["count"], None, None, None)

    for kw, name in ((dict(radius=0.0), b"radius"), (dict(radius=float("nan")), b"radius"),
                     (dict(radius=float("inf")), b"radius"), (dict(min_depth=0.0), b"min_depth"),
                     (dict(zbuf=None), b"zbuf"), (dict(count=None), b"count"), (dict(H=0), b"H="),
                     (dict(n_vertices=-1), b"n_vertices"), (dict(H=1 << 16, W=1 << 15), b"H*W")):
        assert call(**kw) == 1, kw                      # NOF_EINVAL
        assert name in libnof.nof_last_error(), (kw, libnof.nof_last_error())
    # nothing to colour: no launch, and the per-vertex pointers may be missing
    assert call(n_vertices=0, V=None, color_sum=None, count=None) == 0


def test_mesh_carries_counts():
    from bundlesdf_amd.mesh import Mesh
    m = Mesh(np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0]]), np.array([[0, 1, 2], [0, 3, 2]]))
    assert m.vertex_color_counts is None and m.copy().vertex_color_counts is None
    m.vertex_colors = np.arange(12, dtype=np.uint8).reshape(4, 3)
    m.vertex_color_counts = np.array([3, 0, 2, 1], np.int32)
    c = m.copy()
    assert np.array_equal(c.vertex_color_counts, m.vertex_color_counts) and c.vertex_color_counts.dtype == np.int32
    c.vertex_color_counts[0] = 9
    assert m.vertex_color_counts[0] == 3
    c = m.copy().update_vertices([True, False, True, True])
    assert np.array_equal(c.vertex_color_counts, [3, 2, 1]) and np.array_equal(c.vertex_colors, m.vertex_colors[[0, 2, 3]])
    c = m.copy().merge_vertices()            # vertices 1 and 3 coincide: the first occurrence's attributes stay
    assert len(c.vertices) == 3 and sorted(c.vertex_color_counts.tolist()) == [0, 2, 3]
