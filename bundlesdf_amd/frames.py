"""Frame maps on the device: depth clean-up, point and normal maps, match lift, covisibility.

What the tracker does to every incoming frame before RANSAC and the pose graph see anything: the
reference's Frame::processDepth (erodeDepthMap, gaussFilterDepthMap twice), Frame::
depthToCloudAndNormals (convertDepthFloatToCameraSpaceFloat4, computeNormals,
filterDepthSmoothedEdges), Frame::invalidatePixelsByMask, SiftManager::makeCorrespondence and
computeCovisibility. Here they are the five calls of include/nof.h group 10 (csrc/frame_maps.hip),
batched over N frames: float64 arithmetic in a stated order on float32 depth, outputs rounded once,
the same bytes on every run. The header comment of csrc/frame_maps.hip is the definition.

No CPU fallback: every function raises if libnof.so cannot run. FrameMaps.points / .normals are what
optimize_poses(points=, normals=, K=) takes; LiftedMatches.compact() gives the rows ransac_pairs
takes, and LiftedMatches.valid can go to optimize_poses(weight=) as it is.
"""
import ctypes
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._args import as_host, as_tensor, default_device

__all__ = ["prepare_frames", "erode_depth", "bilateral_depth", "depth_geometry", "lift_matches", "covisibility", "relative_poses",
           "FrameMaps", "LiftedMatches", "MAX_RADIUS", "TILE"]

MAX_RADIUS = 8          # FM_MAX_RADIUS of csrc/frame_maps.hip
TILE = (8, 32)          # FM_BY, FM_BX: the rows and columns of pixels one block takes


@dataclass
class FrameMaps:
    """Device tensors of one prepare_frames / depth_geometry call; without the N dimension for a
    single [H,W] frame. stages (with return_stages): the intermediate depth images, in order."""
    depth: torch.Tensor                 # [N,H,W] f32, 0 = no measurement
    points: torch.Tensor                # [N,H,W,3] f32 camera space
    normals: torch.Tensor               # [N,H,W,3] f32, unit or zero
    n_valid: torch.Tensor               # [N] i32: pixels with depth
    K: np.ndarray                       # [3,3] or [N,3,3] f64, as given
    stages: Optional[dict] = None       # "eroded" and "bilateral" (a list, one image per pass)


@dataclass
class LiftedMatches:
    """Device tensors of one lift_matches call, in the row layout of ransac_pairs."""
    pair_frames: torch.Tensor           # [P,2] i32
    pair_start: torch.Tensor            # [P+1] i32
    pts_a: torch.Tensor                 # [M,3] f64, in the camera of the pair's first frame
    pts_b: torch.Tensor                 # [M,3] f64
    normals_a: torch.Tensor             # [M,3] f64
    normals_b: torch.Tensor             # [M,3] f64
    valid: torch.Tensor                 # [M] bool; invalid rows hold zeros
    rows: Optional[torch.Tensor] = None  # [M'] i64 after compact(): the input row of each kept row

    def compact(self):
        """The valid rows alone (torch indexing) with pair_start rebuilt from one host read of the
        flags: what ransac_pairs should get, since it draws hypothesis rows regardless of conf."""
        keep = self.valid.cpu().numpy()
        ps = self.pair_start.cpu().numpy().astype(np.int64)
        csum = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
        idx = torch.from_numpy(np.flatnonzero(keep)).to(self.valid.device)
        return LiftedMatches(pair_frames=self.pair_frames,
                             pair_start=torch.from_numpy(csum[ps].astype(np.int32)).to(self.valid.device),
                             pts_a=self.pts_a[idx], pts_b=self.pts_b[idx], normals_a=self.normals_a[idx],
                             normals_b=self.normals_b[idx],
                             valid=torch.ones(len(idx), dtype=torch.bool, device=self.valid.device), rows=idx)


def _images(a, dtype, what, name):
    """a (array or tensor, [H,W] or [N,H,W]) -> ([N,H,W] tensor of dtype on the device it came from, single)."""
    t = as_tensor(a)
    if t.dim() not in (2, 3):
        raise ValueError(f"{what}: {name} must be [H,W] or [N,H,W], got {tuple(t.shape)}")
    single = t.dim() == 2
    t = t[None] if single else t
    N, H, W = t.shape
    if N < 1 or N > 65535 or H < 1 or W < 1 or N * H * W >= 2 ** 31:
        raise ValueError(f"{what}: {name} of {N}x{H}x{W} (N in 1 .. 65535, H, W at least 1, N*H*W < 2^31)")
    if dtype == torch.uint8:
        t = t != 0
    return t.to(dtype).contiguous(), single


def _radius(r, what, name):
    r = int(r)
    if r < 0 or r > MAX_RADIUS:
        raise ValueError(f"{what}: {name}={r} (0 .. {MAX_RADIUS})")
    return r


def _numbers(what, **kw):
    out = []
    for k, v in kw.items():
        v = float(v)
        if math.isnan(v):
            raise ValueError(f"{what}: {k} is NaN")
        out.append(v)
    return out


def _intrinsics(K, N, what):
    """K [3,3] or [N,3,3], finite, zero skew, the last row (0,0,1) -> [N,4] f64 (fx, fy, cx, cy) on the host."""
    Kh = as_host(K, np.float64)
    if Kh.shape not in ((3, 3), (N, 3, 3)):
        raise ValueError(f"{what}: K must be [3,3] or [{N},3,3], got {Kh.shape}")
    Kn = np.broadcast_to(Kh, (N, 3, 3))
    if not np.isfinite(Kn).all():
        raise ValueError(f"{what}: K is not finite")
    if (Kn[:, 0, 1] != 0).any() or (Kn[:, 1, 0] != 0).any() or (Kn[:, 2] != (0.0, 0.0, 1.0)).any():
        raise ValueError(f"{what}: K must be a pinhole matrix without skew (K[0,1] = K[1,0] = 0, last row 0 0 1)")
    if (Kn[:, 0, 0] == 0).any() or (Kn[:, 1, 1] == 0).any():
        raise ValueError(f"{what}: K has a zero focal length")
    return Kh, np.ascontiguousarray(np.stack([Kn[:, 0, 0], Kn[:, 1, 1], Kn[:, 0, 2], Kn[:, 1, 2]], 1))


def _erode_params(what, radius, diff, ratio, pre=""):
    """erode_depth's own parameters, under the names `pre` gives them -> (radius, what _numbers has still to
    check). Every caller validates in two steps, all integers and then all numbers, so that a refusal
    does not depend on which stage an argument belongs to."""
    return _radius(radius, what, pre + "radius"), {pre + "diff": diff, pre + "ratio": ratio}


def _bilateral_params(what, radius, passes, sigma_d, sigma_r, band, pre=""):
    """bilateral_depth's own parameters -> (radius, passes, what _numbers has still to check); _sigmas follows it."""
    radius = _radius(radius, what, pre + "radius")
    passes = int(passes)
    if passes < 0:
        raise ValueError(f"{what}: {pre}passes={passes} must not be negative")
    return radius, passes, {"sigma_d": sigma_d, "sigma_r": sigma_r, pre + "band": band}


def _sigmas(what, sigma_d, sigma_r):
    if not sigma_d > 0 or not sigma_r > 0:
        raise ValueError(f"{what}: sigma_d={sigma_d} and sigma_r={sigma_r} must be positive")


def _geometry_params(what, d, K, mask, z_diff, edge_angle_deg):
    """depth_geometry's own parameters for the depth images d [N,H,W] -> (K as given in f64, [N,4] f64, the mask
    [N,H,W] u8 or None, what _numbers has still to check)."""
    Kh, K4 = _intrinsics(K, d.shape[0], what)
    m = None
    if mask is not None:
        m, _ = _images(mask, torch.uint8, what, "mask")
        if m.shape != d.shape:
            raise ValueError(f"{what}: mask is {tuple(m.shape)}, depth {tuple(d.shape)}")
    return Kh, K4, m, {"z_diff": z_diff, "edge_angle_deg": edge_angle_deg}


def _erode(L, d, radius, depth_min, zfar, diff, ratio):
    out = torch.empty_like(d)
    D = _lib.FrameErodeDesc()
    D.in_, D.out = _lib.ptr(d), _lib.ptr(out)
    D.N, D.H, D.W = d.shape
    D.radius, D.depth_min, D.zfar, D.diff, D.ratio = radius, depth_min, zfar, diff, ratio
    _lib.check(L.nof_frame_erode(ctypes.byref(D), _lib.stream_of(d)), "erode_depth")
    return out


def _bilateral(L, d, radius, depth_min, zfar, sigma_d, sigma_r, band):
    out = torch.empty_like(d)
    D = _lib.FrameBilateralDesc()
    D.in_, D.out = _lib.ptr(d), _lib.ptr(out)
    D.N, D.H, D.W = d.shape
    D.radius, D.depth_min, D.zfar, D.band = radius, depth_min, zfar, band
    D.two_sigma_d_sq, D.two_sigma_r_sq = 2.0 * sigma_d * sigma_d, 2.0 * sigma_r * sigma_r
    _lib.check(L.nof_frame_bilateral(ctypes.byref(D), _lib.stream_of(d)), "bilateral_depth")
    return out


def _geometry(L, d, K4, mask, depth_min, z_diff, sin_edge):
    N, H, W = d.shape
    dev = d.device
    depth = torch.empty_like(d)
    points = torch.empty((N, H, W, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((N, H, W, 3), dtype=torch.float32, device=dev)
    n_valid = torch.empty(N, dtype=torch.int32, device=dev)
    Kd = torch.from_numpy(K4).to(dev)
    D = _lib.FrameGeometryDesc()
    D.depth_in, D.K, D.mask = _lib.ptr(d), _lib.ptr(Kd), _lib.ptr(mask)
    D.N, D.H, D.W = N, H, W
    D.depth_min, D.z_diff, D.sin_edge = depth_min, z_diff, sin_edge
    D.depth, D.points, D.normals, D.n_valid = (_lib.ptr(x) for x in (depth, points, normals, n_valid))
    _lib.check(L.nof_frame_geometry(ctypes.byref(D), _lib.stream_of(d)), "depth_geometry")
    return depth, points, normals, n_valid


def erode_depth(depth, *, zfar=1.0, depth_min=0.1, radius=1, diff=0.001, ratio=0.8, device=None):
    """erodeDepthMap: a pixel survives if depth_min < c <= zfar and fewer than ratio of its (2 radius +
    1)^2 window are bad (below depth_min, or further than diff from c; taps outside the image are not
    counted). depth [H,W] or [N,H,W] -> a float32 device tensor of the same shape."""
    what = "erode_depth"
    d, single = _images(depth, torch.float32, what, "depth")
    radius, numbers = _erode_params(what, radius, diff, ratio)
    depth_min, zfar, diff, ratio = _numbers(what, depth_min=depth_min, zfar=zfar, **numbers)
    dev = default_device(d, device)
    L = _lib.lib()
    with torch.cuda.device(dev):
        out = _erode(L, d.to(dev), radius, depth_min, zfar, diff, ratio)
    return out[0] if single else out


def bilateral_depth(depth, *, zfar=1.0, depth_min=0.1, radius=2, sigma_d=2.0, sigma_r=1e5, band=0.01, passes=2,
                    device=None, return_passes=False):
    """gaussFilterDepthMap, `passes` times: the Gaussian-weighted mean of the usable taps within band
    of the window's mean depth. Holes are filled and the silhouette grows by radius per pass, as in the
    reference. With return_passes the image after every pass comes back as a list."""
    what = "bilateral_depth"
    d, single = _images(depth, torch.float32, what, "depth")
    radius, passes, numbers = _bilateral_params(what, radius, passes, sigma_d, sigma_r, band)
    depth_min, zfar, sigma_d, sigma_r, band = _numbers(what, depth_min=depth_min, zfar=zfar, **numbers)
    _sigmas(what, sigma_d, sigma_r)
    dev = default_device(d, device)
    L = _lib.lib()
    outs = []
    with torch.cuda.device(dev):
        d = d.to(dev)
        for _ in range(passes):
            d = _bilateral(L, d, radius, depth_min, zfar, sigma_d, sigma_r, band)
            outs.append(d[0] if single else d)
    d = d[0] if single else d
    return (d, outs) if return_passes else d


def depth_geometry(depth, K, mask=None, *, depth_min=0.1, z_diff=0.02, edge_angle_deg=10.0, device=None):
    """Points, normals, the grazing-angle filter and the mask -> FrameMaps. K [3,3] or [N,3,3] without
    skew; mask [H,W] or [N,H,W] of any dtype, 0 drops the pixel."""
    what = "depth_geometry"
    d, single = _images(depth, torch.float32, what, "depth")
    Kh, K4, m, numbers = _geometry_params(what, d, K, mask, z_diff, edge_angle_deg)
    depth_min, z_diff, edge = _numbers(what, depth_min=depth_min, **numbers)
    dev = default_device(d, device)
    L = _lib.lib()
    with torch.cuda.device(dev):
        out = _geometry(L, d.to(dev), K4, None if m is None else m.to(dev), depth_min, z_diff,
                        math.sin(math.radians(edge)))
    if single:
        out = tuple(x[0] for x in out)
    return FrameMaps(*out, K=Kh)


def prepare_frames(depth, K, mask=None, *, zfar=1.0, depth_min=0.1, erode_radius=1, erode_diff=0.001, erode_ratio=0.8,
                   bilateral_radius=2, sigma_d=2.0, sigma_r=1e5, bilateral_band=0.01, bilateral_passes=2, z_diff=0.02,
                   edge_angle_deg=10.0, return_stages=False, device=None):
    """Raw depth frames [N,H,W] (or one [H,W]) in metres -> FrameMaps: erode_depth, bilateral_depth and
    depth_geometry in a row on the current stream, nothing read back in between; every argument is
    validated before the first launch. The defaults are the depth_processing block of the reference's
    BundleTrack/config_ho3d.yml. With return_stages, FrameMaps.stages holds "eroded" and "bilateral"
    (one image per pass)."""
    what = "prepare_frames"
    d, single = _images(depth, torch.float32, what, "depth")
    Kh, K4, m, g_numbers = _geometry_params(what, d, K, mask, z_diff, edge_angle_deg)
    er, e_numbers = _erode_params(what, erode_radius, erode_diff, erode_ratio, "erode_")
    br, passes, b_numbers = _bilateral_params(what, bilateral_radius, bilateral_passes, sigma_d, sigma_r, bilateral_band,
                                              "bilateral_")
    depth_min, zfar, diff, ratio, sigma_d, sigma_r, band, z_diff, edge = _numbers(
        what, depth_min=depth_min, zfar=zfar, **e_numbers, **b_numbers, **g_numbers)
    _sigmas(what, sigma_d, sigma_r)
    dev = default_device(d, device)
    L = _lib.lib()
    with torch.cuda.device(dev):
        e = b = _erode(L, d.to(dev), er, depth_min, zfar, diff, ratio)
        outs = []
        for _ in range(passes):
            b = _bilateral(L, b, br, depth_min, zfar, sigma_d, sigma_r, band)
            outs.append(b)
        out = _geometry(L, b, K4, None if m is None else m.to(dev), depth_min, z_diff, math.sin(math.radians(edge)))
    if single:
        out, e, outs = tuple(x[0] for x in out), e[0], [x[0] for x in outs]
    maps = FrameMaps(*out, K=Kh)
    if return_stages:
        maps.stages = dict(eroded=e, bilateral=outs)
    return maps


def relative_poses(poses, pairs):
    """T[q] = inv(pose_b) pose_a for pairs[q] = (a, b), float64 on the host with the inverse taken as
    R^T, -R^T t: R = Rb^T Ra and t = Rb^T ta + (-(Rb^T tb)), every sum of three products as (x + y) + z."""
    Th = np.asarray(poses, np.float64)
    pf = np.asarray(pairs, np.int64).reshape(-1, 2)
    A, B = Th[pf[:, 0]], Th[pf[:, 1]]
    T = np.tile(np.eye(4), (len(pf), 1, 1))
    for i in range(3):
        for j in range(3):
            T[:, i, j] = (B[:, 0, i] * A[:, 0, j] + B[:, 1, i] * A[:, 1, j]) + B[:, 2, i] * A[:, 2, j]
        ti = -((B[:, 0, i] * B[:, 0, 3] + B[:, 1, i] * B[:, 1, 3]) + B[:, 2, i] * B[:, 2, 3])
        T[:, i, 3] = ((B[:, 0, i] * A[:, 0, 3] + B[:, 1, i] * A[:, 1, 3]) + B[:, 2, i] * A[:, 2, 3]) + ti
    return T


def _maps(maps, what):
    """(points, normals) [N,H,W,3] f32 contiguous device tensors of a FrameMaps (a single frame counts as N = 1)."""
    p, n = maps.points, maps.normals
    if p.dim() == 3:
        p, n = p[None], n[None]
    if p.dim() != 4 or p.shape[-1] != 3 or n.shape != p.shape or p.dtype != torch.float32 or n.dtype != torch.float32:
        raise ValueError(f"{what}: maps.points and maps.normals must be float32 [N,H,W,3], got {tuple(p.shape)} "
                         f"and {tuple(n.shape)}")
    return p.detach().contiguous(), n.detach().contiguous()


def _poses(poses, N, what):
    T = as_tensor(poses)
    if tuple(T.shape) != (N, 4, 4):
        raise ValueError(f"{what}: poses must be [{N},4,4], got {tuple(T.shape)}")
    return T.to(torch.float64).contiguous()


def _pairs(pairs, N, what, name, lo, allow_self):
    pf = as_host(pairs, np.int64)
    if pf.ndim != 2 or pf.shape[1] != 2:
        raise ValueError(f"{what}: {name} must be [*,2], got {pf.shape}")
    if len(pf) < lo or len(pf) > 65535:
        raise ValueError(f"{what}: {len(pf)} pairs ({lo} .. 65535)")
    if (pf < 0).any() or (pf >= N).any():
        raise ValueError(f"{what}: {name} has a frame index outside 0 .. {N - 1}")
    if not allow_self and (pf[:, 0] == pf[:, 1]).any():
        raise ValueError(f"{what}: {name} has a pair of a frame with itself")
    return pf


def lift_matches(maps, pair_frames, uv_a, uv_b, pair_start=None, *, poses=None, max_dist=None, max_normal_deg=None,
                 depth_min=0.1):
    """Pixel matches -> LiftedMatches (SiftManager::makeCorrespondence). uv_a / uv_b [M,2] hold (u, v) =
    (column, row) in the two frames of each row's pair; pair p = pair_frames[p] owns the rows
    pair_start[p] .. pair_start[p+1]-1 (None: one pair). Coordinates are rounded half away from zero
    and then bounds-checked; a row is valid if both pixels exist with z > depth_min and, with poses
    [N,4,4] (camera in world), the world distance is at most max_dist and the world normals are within
    max_normal_deg of each other (None: no such gate)."""
    what = "lift_matches"
    pts, nrm = _maps(maps, what)
    N, H, W = pts.shape[:3]
    pf = _pairs(pair_frames, N, what, "pair_frames", 1, True)
    P = len(pf)

    def rows(a, name):
        t = as_tensor(a, np.float64)
        if t.dim() != 2 or t.shape[1] != 2:
            raise ValueError(f"{what}: {name} must be [M,2], got {tuple(t.shape)}")
        return t.to(torch.float64).contiguous()

    ua, ub = rows(uv_a, "uv_a"), rows(uv_b, "uv_b")
    M = len(ua)
    if len(ub) != M:
        raise ValueError(f"{what}: uv_a has {M} rows, uv_b {len(ub)}")
    if M >= 2 ** 31:
        raise ValueError(f"{what}: {M} rows (max 2^31 - 1)")
    if pair_start is None:
        if P != 1:
            raise ValueError(f"{what}: pair_start is needed for {P} pairs")
        ps = np.array([0, M], np.int64)
    else:
        ps = as_host(pair_start, np.int64).reshape(-1)
    if ps.shape != (P + 1,) or ps[0] != 0 or ps[-1] != M or (np.diff(ps) < 0).any():
        raise ValueError(f"{what}: pair_start must be [{P + 1}], start at 0, never decrease and end at M={M}")
    if poses is None and (max_dist is not None or max_normal_deg is not None):
        raise ValueError(f"{what}: max_dist and max_normal_deg need poses")
    T = None if poses is None else _poses(poses, N, what)
    (depth_min,) = _numbers(what, depth_min=depth_min)
    gate_dist = gate_normal = 0
    dist = cosn = 0.0
    if max_dist is not None:
        (dist,), gate_dist = _numbers(what, max_dist=max_dist), 1
    if max_normal_deg is not None:
        (deg,), gate_normal = _numbers(what, max_normal_deg=max_normal_deg), 1
        cosn = math.cos(math.radians(deg))

    dev = default_device(pts)
    L = _lib.lib()
    f64 = torch.float64
    with torch.cuda.device(dev):
        pts, nrm, ua, ub = pts.to(dev), nrm.to(dev), ua.to(dev), ub.to(dev)
        T = None if T is None else T.to(dev)
        out = LiftedMatches(pair_frames=torch.from_numpy(pf.astype(np.int32)).to(dev),
                            pair_start=torch.from_numpy(ps.astype(np.int32)).to(dev),
                            pts_a=torch.empty((M, 3), dtype=f64, device=dev), pts_b=torch.empty((M, 3), dtype=f64, device=dev),
                            normals_a=torch.empty((M, 3), dtype=f64, device=dev),
                            normals_b=torch.empty((M, 3), dtype=f64, device=dev),
                            valid=torch.empty(M, dtype=torch.uint8, device=dev))
        D = _lib.FrameLiftDesc()
        D.points, D.normals, D.N, D.H, D.W, D.P, D.M = _lib.ptr(pts), _lib.ptr(nrm), N, H, W, P, M
        D.pair_frames, D.pair_start, D.uv_a, D.uv_b, D.poses = (_lib.ptr(x) for x in (out.pair_frames, out.pair_start,
                                                                                        ua, ub, T))
        D.depth_min, D.max_dist, D.cos_normal, D.gate_dist, D.gate_normal = depth_min, dist, cosn, gate_dist, gate_normal
        D.pts_a, D.pts_b, D.normals_a, D.normals_b, D.valid = (_lib.ptr(x) for x in (out.pts_a, out.pts_b, out.normals_a,
                                                                                      out.normals_b, out.valid))
        _lib.check(L.nof_frame_lift_matches(ctypes.byref(D), _lib.stream_of(pts)), what)
        out.valid = out.valid.bool()
    return out


def covisibility(maps, poses, pairs, *, visible_angle_deg=70.0, stride=2, depth_min=0.1):
    """computeCovisibility for Q ordered pairs (a, b) -> (ratio [Q] f64, counts [Q,2] i32 = visible,
    total), device tensors. Over every stride-th pixel of frame a (from pixel (0,0)) that has depth and
    a normal: visible if, seen from frame b (T = inv(pose_b) pose_a, formed here in float64 as R^T, -R^T
    t), the direction to the eye and the normal are within visible_angle_deg. ratio = visible / (total +
    1e-7), formed in torch."""
    what = "covisibility"
    pts, nrm = _maps(maps, what)
    N, H, W = pts.shape[:3]
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"{what}: stride={stride} must be at least 1")
    pf = _pairs(pairs, N, what, "pairs", 0, True)
    Q = len(pf)
    Th = _poses(poses, N, what).cpu().numpy()
    depth_min, ang = _numbers(what, depth_min=depth_min, visible_angle_deg=visible_angle_deg)
    T = np.ascontiguousarray(relative_poses(Th, pf))
    dev = default_device(pts)
    L = _lib.lib()
    with torch.cuda.device(dev):
        pts, nrm = pts.to(dev), nrm.to(dev)
        counts = torch.zeros((Q, 2), dtype=torch.int32, device=dev)
        if Q:
            pd, Td = torch.from_numpy(pf.astype(np.int32)).to(dev), torch.from_numpy(T).to(dev)
            D = _lib.FrameCovisDesc()
            D.points, D.normals, D.N, D.H, D.W, D.Q = _lib.ptr(pts), _lib.ptr(nrm), N, H, W, Q
            D.pairs, D.T, D.stride, D.depth_min, D.cos_visible = _lib.ptr(pd), _lib.ptr(Td), stride, depth_min, \
                math.cos(math.radians(ang))
            D.counts = _lib.ptr(counts)
            _lib.check(L.nof_frame_covisibility(ctypes.byref(D), _lib.stream_of(pts)), what)
        ratio = counts[:, 0].double() / (counts[:, 1].double() + 1e-7)
    return ratio, counts
